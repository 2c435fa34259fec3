// group16.h -- reductions across the 16 lanes of a wave that share a row of
// the classifier tile (one class group, lanes l & 15 of gemm_tile.h's
// mapping): the row epilogues of xent_fwd_kernel (xent_fwd.h) and
// eval_fwd_kernel (eval.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace sgc {

namespace {

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

}  // namespace
}  // namespace sgc
