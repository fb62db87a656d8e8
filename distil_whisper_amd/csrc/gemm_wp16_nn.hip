// gemm_wp16.h (v_mfma_f32_16x16x32_bf16 main loop), row-major operands, 256-row block tile
#include "gemm_wp16.h"
int dw_gemm_wp16_nn_launch(const GemmP& p, hipStream_t s) { return launch_wp16<false, false, 256>(p, s); }
