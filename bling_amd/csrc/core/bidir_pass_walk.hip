// bidir_pass_walk.hip -- k_bd_walk for every scene feature (FT_ALL); see bidir_pass.hip.
#define BLING_BIDIR_UNIT_WALK_ALL 1
#include "bidir_pass.hip"
