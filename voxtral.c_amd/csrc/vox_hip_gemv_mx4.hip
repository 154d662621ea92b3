// vox_hip_gemv_mx4.hip -- the k_gemv and k_gemvr instances that stream wmx4 plane (vox_wmx4.h).
#include "vox_hip_gemv_pick.h"

VOX_GEMV_FORMAT(vox::WF_MX4, mx4)
