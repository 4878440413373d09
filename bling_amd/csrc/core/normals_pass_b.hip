// normals_pass_b.hip -- the normal-map kernels of feature profiles kProfiles[3] and [4]; see normals_pass.hip.
#define BLING_NM_UNIT 1
#include "normals_pass.hip"
