// adam_update.h -- the element update of torch.optim.Adam's default
// single-tensor path (amsgrad=False, maximize=False, coupled L2 weight decay),
// shared by adam.hip and the fused epilogue in xent.hip.  The operation order
// is the contract written in include/sgc_amd.h.
#pragma once

#include "common.h"

namespace sgc {

// Per-step constants, computed on the host in double and rounded to fp32 once.
struct AdamCoef {
    float wd;         // weight_decay (0: the decay term is skipped)
    float omb1;       // 1 - beta1
    float b2;         // beta2
    float omb2;       // 1 - beta2
    float bc2_sqrt;   // sqrt(1 - beta2^step)
    float eps;
    float step_size;  // lr / (1 - beta1^step)
};

// One rounding per operation (the library is built with -ffp-contract=off;
// sqrtf and the divisions are correctly rounded).
__device__ __forceinline__ void adam_update(float &p, float &m, float &v, float g,
                                            const AdamCoef &c) {
    if (c.wd != 0.f) g = g + c.wd * p;
    m = m + (g - m) * c.omb1;
    v = c.b2 * v + (c.omb2 * g) * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p - c.step_size * (m / denom);
}

// The constants of Adam step `step` (>= 1).
AdamCoef adam_coef(int64_t step, double lr, double beta1, double beta2, double eps,
                   double weight_decay);

// (xent.hip's xent_adam_epoch / xent_adam_check: internal.h)

}  // namespace sgc
