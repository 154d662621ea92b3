// vox_hip_gemv_bf16.hip -- the k_gemv and k_gemvr instances that stream bf16 rows.
#include "vox_hip_gemv_pick.h"

VOX_GEMV_FORMAT(vox::WF_BF16, bf16)
