// xent_fwd_stop.hip -- launch A of the fused classifier step behind the L-BFGS
// state's stop word, for the closures of sgc_train_lbfgs_f32 (lbfgs.hip):
// xent_fwd_kernel<V, NT, NB, StopWord> (xent_fwd.h), which takes the word as
// its last argument and returns after one wave-uniform load at entry when it is
// set.  It is a unit of its own so that xent.hip's code object holds the
// NoStop instantiations alone.
#include "internal.h"
#include "xent_fwd.h"

namespace sgc {

hipError_t launch_xent_fwd_stop(int V, int NT, const int64_t *stop, const float *X, int64_t ldx,
                                const float *W, const float *b, const int64_t *labels, int M, int K,
                                int C, float *G, int ldg, double *loss_part, float *db_part,
                                float *logits, int64_t ldl, hipStream_t s) {
    return launch_xent_fwd(StopWord{stop}, V, NT, g_tile_buffers, X, ldx, W, b, labels, M, K, C, G,
                           ldg, loss_part, db_part, logits, ldl, s);
}

SGC_WARM_UNIT(warm_xent_fwd_stop)

}  // namespace sgc
