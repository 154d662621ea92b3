# The kernel translation units, csrc/NAME.hip, one per kernel family: named once,
# here, for the product's Makefile and for tools/Makefile.  Heaviest first, so that a parallel
# build starts them first.
VOX_KERNEL_UNITS := vox_hip_gemv_bf16 vox_hip_gemv_q8 vox_hip_gemv_p13 vox_hip_gemv_mx4 \
                    vox_hip_kernels vox_hip_gemmf vox_hip_gemv
