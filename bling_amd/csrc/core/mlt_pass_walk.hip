// mlt_pass_walk.hip -- k_mlt_walk for every scene feature (FT_ALL); see mlt_pass.hip.
#define BLING_MLT_UNIT_WALK_ALL 1
#include "mlt_pass.hip"
