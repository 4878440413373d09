// normals_pass_c.hip -- the normal-map kernels of feature profile kProfiles[5]; see normals_pass.hip.
#define BLING_NM_UNIT 2
#include "normals_pass.hip"
