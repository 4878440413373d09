// bidir_pass_connect.hip -- k_bd_connect for every scene feature (FT_ALL); see bidir_pass.hip.
#define BLING_BIDIR_UNIT_CONNECT_ALL 1
#include "bidir_pass.hip"
