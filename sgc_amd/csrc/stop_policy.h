// stop_policy.h -- whether a kernel of the fused classifier step runs behind
// the L-BFGS state's stop word (sgc_train_lbfgs_f32, lbfgs.hip).  A kernel
// takes the policy as its last template parameter and its last argument, and
// begins with `if (stop.set()) return;`.
//   NoStop    the plain kernel: an empty argument (no kernarg bytes, every
//             other argument where it was) and a test that folds away;
//   StopWord  one wave-uniform load of the device word at entry; the kernel
//             returns when it is set.
// The kernel stays the unit the compiler optimises: one text, two
// instantiations, no inlined body ("One text, two kernels").
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sgc {

struct NoStop {
    __device__ bool set() const { return false; }
};
struct StopWord {
    const int64_t *w;
    __device__ bool set() const { return *w != 0; }
};

}  // namespace sgc
