// eval.h -- the argmax rule of the evaluation kernels (eval.hip, eval16.hip):
// torch's max(1)[1].  A row's prediction is the smallest class index whose
// logit no other class exceeds, a NaN counts as greater than everything (the
// first NaN wins), -0 and +0 tie, and a padded class (>= C) never wins.
//
// The rule is one unsigned maximum: a (logit, class) pair becomes a 64-bit key
// whose high word orders the logit (NaN on top, then +inf ... -inf) and whose
// low word is the complemented class index, so among equal logits the smallest
// index has the largest key.  The key of "no class" is 0, below every real
// class (the low word of a real class is never 0).  A maximum is associative
// and commutative, so the result does not depend on how the lanes, class
// tiles and shuffles are ordered.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgc {

__device__ __forceinline__ unsigned long long argmax_key(float z, int c) {
    const uint32_t u = __float_as_uint(z + 0.0f);  // -0 -> +0: torch compares them equal
    const uint32_t ord = (z != z) ? 0xffffffffu : (u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
    return ((unsigned long long)ord << 32) | (uint32_t)~(uint32_t)c;
}

__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) {
    return a > b ? a : b;
}

__device__ __forceinline__ int key_class(unsigned long long k) { return (int)~(uint32_t)k; }

}  // namespace sgc
