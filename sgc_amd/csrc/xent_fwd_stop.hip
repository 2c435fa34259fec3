// xent_fwd_stop.hip -- launch A of the fused classifier step (xent.hip:
// xent_fwd_kernel) behind the L-BFGS state's stop word, for the closures of
// sgc_train_lbfgs_f32 (lbfgs.hip).  The kernel is xent.hip's own text, included
// with SGC_XENT_STOP_PASS 1: `stop` becomes its first argument and one
// wave-uniform load at entry returns when the word is set.  It is a unit of
// its own so that xent.hip's code object holds the plain kernels alone.
#include "gemm_tile.h"
#include "internal.h"

#define SGC_XENT_KERNEL(name) name##_stop_kernel
#define SGC_XENT_STOP_PARAM const int64_t *__restrict__ stop,
#define SGC_XENT_STOP_TEST \
    if (*stop != 0) return;
#define SGC_XENT_STOP_PASS 1

namespace sgc {

namespace {
#include "xent.hip"
}  // namespace

hipError_t launch_xent_fwd_stop(int V, int NT, const int64_t *stop, const float *X, int64_t ldx,
                                const float *W, const float *b, const int64_t *labels, int M, int K,
                                int C, float *G, int ldg, double *loss_part, float *db_part,
                                float *logits, int64_t ldl, hipStream_t s) {
    const int blocks = (M + kLdsBM - 1) / kLdsBM;
    const float inv_m = 1.0f / (float)M;
#define SGC_FWD_STOP(VV, NN)                                                                      \
    if (g_tile_buffers == 1)                                                                      \
        hipLaunchKernelGGL((xent_fwd_stop_kernel<VV, NN, 1>), dim3(blocks), dim3(256), 0, s, stop, \
                           X, ldx, W, b, labels, M, K, C, inv_m, G, ldg, loss_part, db_part,      \
                           logits, ldl);                                                          \
    else                                                                                          \
        hipLaunchKernelGGL((xent_fwd_stop_kernel<VV, NN, 2>), dim3(blocks), dim3(256), 0, s, stop, \
                           X, ldx, W, b, labels, M, K, C, inv_m, G, ldg, loss_part, db_part,      \
                           logits, ldl);                                                          \
    break;
#define SGC_FWD_STOP_NT(VV)              \
    switch (NT) {                        \
        case 1: SGC_FWD_STOP(VV, 1)      \
        case 2: SGC_FWD_STOP(VV, 2)      \
        case 3: SGC_FWD_STOP(VV, 3)      \
        default: SGC_FWD_STOP(VV, 4)     \
    }
    if (V == 4) {
        SGC_FWD_STOP_NT(4)
    } else if (V == 2) {
        SGC_FWD_STOP_NT(2)
    } else {
        SGC_FWD_STOP_NT(1)
    }
#undef SGC_FWD_STOP_NT
#undef SGC_FWD_STOP
    return hipGetLastError();
}

SGC_WARM_UNIT(warm_xent_fwd_stop)

}  // namespace sgc
