// x16.h -- 16-bit feature elements (bfloat16 / float16 in memory, fp32 in
// registers) for the SpMM kernels: exact widening, one round-to-nearest-even
// per stored element.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgc {

struct bf16_t { uint16_t u; };  // torch.bfloat16's bits
struct f16_t { uint16_t u; };   // torch.float16's bits

// The low 16 bits of `bits` as T, widened to fp32 (exact; subnormals kept).
template <typename T> __device__ __forceinline__ float widen16(uint32_t bits);
template <> __device__ __forceinline__ float widen16<bf16_t>(uint32_t bits) {
    return __uint_as_float(bits << 16);
}
template <> __device__ __forceinline__ float widen16<f16_t>(uint32_t bits) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);  // v_cvt_f32_f16
}

// Both halves of one dword (element 2i in the low half, little endian).
template <typename T> __device__ __forceinline__ void widen16x2(uint32_t w, float &lo, float &hi) {
    lo = widen16<T>(w);
    hi = widen16<T>(w >> 16);
}
template <> __device__ __forceinline__ void widen16x2<bf16_t>(uint32_t w, float &lo, float &hi) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xffff0000u);
}

// fp32 -> T, round to nearest even: the bits of torch's CPU tensor.to(T) for
// every finite x (subnormal results and fp16 overflow to +-inf included);
// NaN stays NaN.  bf16 in integer arithmetic (the carry into the exponent is
// the rounding up to the next binade or to inf), fp16 by v_cvt_f16_f32.
template <typename T> __device__ __forceinline__ uint32_t round16(float x);
template <> __device__ __forceinline__ uint32_t round16<bf16_t>(float x) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x0040u;  // quiet NaN, sign kept
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
template <> __device__ __forceinline__ uint32_t round16<f16_t>(float x) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);
}

// One element in memory as fp32 / fp32 into one element in memory.
template <typename T> __device__ __forceinline__ float load_elem(const void *p) {
    if constexpr (sizeof(T) == 4)
        return *reinterpret_cast<const float *>(p);
    else
        return widen16<T>(*reinterpret_cast<const uint16_t *>(p));
}
template <typename T> __device__ __forceinline__ void store_elem(T *p, float x) {
    if constexpr (sizeof(T) == 4)
        *p = x;
    else
        p->u = (uint16_t)round16<T>(x);
}

}  // namespace sgc
