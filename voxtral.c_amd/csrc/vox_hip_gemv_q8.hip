// vox_hip_gemv_q8.hip -- the k_gemv and k_gemvr instances that stream Q8 rows + row scales.
#include "vox_hip_gemv_pick.h"

VOX_GEMV_FORMAT(vox::WF_Q8, q8)
