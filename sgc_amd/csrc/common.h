// common.h -- shared helpers for the gfx950 kernels of libsgc_amd.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgc_amd.h"

namespace sgc {

// Thread-local message for sgc_last_error().
void set_error(const char *fmt, ...);

#define SGC_HIP_CHECK(expr)                                                         \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            ::sgc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                             __FILE__, __LINE__);                                   \
            return SGC_EHIP;                                                        \
        }                                                                           \
    } while (0)

#define SGC_REQUIRE(cond, code, ...)       \
    do {                                   \
        if (!(cond)) {                     \
            ::sgc::set_error(__VA_ARGS__); \
            return (code);                 \
        }                                  \
    } while (0)

static constexpr int kWave = 64;  // CDNA wavefront width (never 32)

// Code-object warm-up (sgc_warmup): the runtime loads a translation unit's
// code object on the first launch of any of its kernels, so one empty launch
// per unit moves that load out of the first real call.  SGC_WARM_UNIT(name)
// defines `hipError_t name(hipStream_t)` launching this unit's empty kernel.
#define SGC_WARM_UNIT(name)                                                 \
    namespace {                                                             \
    __global__ void name##_kernel() {}                                      \
    }                                                                       \
    hipError_t name(hipStream_t s) {                                        \
        hipLaunchKernelGGL(name##_kernel, dim3(1), dim3(kWave), 0, s);      \
        return hipGetLastError();                                           \
    }
// (each unit's warm-up is declared in internal.h)

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// V consecutive fp32 in one lane: float / float2 / float4 register vectors,
// loaded with one global_load_dword{,x2,x4}.
template <int V> struct Vec { typedef float __attribute__((ext_vector_type(V))) T; };
template <> struct Vec<1> { typedef float T; };

template <int V>
__device__ __forceinline__ float lane_elem(const typename Vec<V>::T &x, int i) { return x[i]; }
template <>
__device__ __forceinline__ float lane_elem<1>(const float &x, int) { return x; }

template <int V>
__device__ __forceinline__ void set_elem(typename Vec<V>::T &x, int i, float v) { x[i] = v; }
template <>
__device__ __forceinline__ void set_elem<1>(float &x, int, float v) { x = v; }

// The same vectors at 4-byte alignment: gfx950 runs with unaligned access
// enabled, so an access through this type is still one
// global_{load,store}_dwordx{2,4} (a caller's [N, 602] rows are 2,408 B
// apart: 8-B aligned at best).
template <int V> struct VecU { typedef float __attribute__((ext_vector_type(V), aligned(4))) T; };
template <> struct VecU<1> { typedef float T; };

// Columns f .. f+V-1 of a row that ends at column F and is only 4-byte
// aligned: one V-wide access when the lane's vector lies wholly below F, the
// scalar bounds-checked form for the one lane that straddles F (columns at or
// beyond F are never touched; load_upto leaves them +0.0f).
template <int V>
__device__ __forceinline__ typename Vec<V>::T load_upto(const float *row, int f, int F) {
    typename Vec<V>::T x;
    if (f + V <= F) {
        x = *reinterpret_cast<const typename VecU<V>::T *>(row + f);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) set_elem<V>(x, v, f + v < F ? row[f + v] : 0.0f);
    }
    return x;
}

template <int V>
__device__ __forceinline__ void store_upto(float *row, int f, int F, const typename Vec<V>::T &x) {
    if (f + V <= F) {
        *reinterpret_cast<typename VecU<V>::T *>(row + f) = x;
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (f + v < F) row[f + v] = lane_elem<V>(x, v);
    }
}

}  // namespace sgc
