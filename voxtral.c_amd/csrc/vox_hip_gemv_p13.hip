// vox_hip_gemv_p13.hip -- the k_gemv and k_gemvr instances that stream wpack13 planes (vox_wpack.h).
#include "vox_hip_gemv_pick.h"

VOX_GEMV_FORMAT(vox::WF_P13, p13)
