// linear16.hip -- the SGC classifier on 16-bit features (torch.bfloat16 /
// torch.float16 X; W, b, dY, the logits, dW and db fp32): the forward
// Y = float(X) . W^T + b and the weight backward dW = dY^T . float(X),
// db = sum dY, beside the fp32 kernels of linear.hip / xent.hip as spmm16.hip
// stands beside spmm.hip.  Every result is defined on the exactly widened
// elements; nothing is rounded to 16 bits anywhere.
//
// The split-bf16 scheme of split_bf16.h with these pieces (x piece, w piece):
//   W and dY are split in three (h, m, l) as in the fp32 kernels;
//   a bf16 x is its own single piece h = x: hh into accH, hm and hl into accL,
//     nothing dropped (3 MFMAs per class tile, no split of X);
//   an fp16 x is exactly two pieces, h = RNE_bf16(x) and m = x - h (11
//     significant bits fit in 8 + 3; fp16 subnormals are normal bf16 values):
//     hh into accH, hm, mh, hl, mm into accL; the dropped ml is the term the
//     fp32 scheme drops too (5 MFMAs per class tile).
// Non-finite x inside the K range gives non-finite results in its row of Y /
// its column of dW, not necessarily torch's +-inf (an infinite fp16 x has
// m = inf - inf; an infinite x times a zero piece of w is NaN) -- the
// deviation documented for the fp32 split kernels.  Padding past K may hold
// anything: it is zeroed in registers (forward) or reaches only columns that
// are never stored (backward).
//
// Layout preconditions of both kernels: element pitch even and base 4-B
// aligned (every buffer range is then a whole number of dwords; b128 / b64
// buffer loads run at 4-B alignment, as the fp32 split kernel's do at odd
// pitches), and M * ldx * 2 < 2^31.
#include <algorithm>

#include "x16_stream.h"

namespace sgc {

// ---------------------------------------------------------------------------
// Forward: x16::stream (x16_stream.h) with finished tiles held and stored
// after the stream, classes 64 at a time.
template <int NT, int NW, typename XT>
__global__ __launch_bounds__(64 * NW) void linear_x16_kernel(
    const XT *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, float *__restrict__ Y, int64_t ldy, int M, int K, int C) {
    using namespace x16;
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) u32x4 sgr16[];
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, kg = lane >> 4;
    const auto yd = __builtin_amdgcn_make_buffer_rsrc(Y, 0, (int)((int64_t)M * ldy * 4),
                                                      0x00020000);  // < 2^31
    // (more than kHeld at NT <= 2 put the held tiles in scratch)
    constexpr int PT0 = NT <= 3 ? kHeld : kHeld - 2;
    constexpr int PT = PT0 < 1 ? 1 : PT0;
    f4 held[PT][NT];
    uint32_t hrow[PT];
    int nheld = 0;  // uniform
    const int pcl = (NT - 1) * 16 + 4 * kg;  // the lane's last class group
    const bool ppart = pcl + 4 > C;           // partial (or empty): b32 stores
    // Y row offset -> its classes: full groups of four by b128, the partial
    // last group by b32; every store issued, out-of-range offsets when empty
    auto store_tile = [&](const f4 (&o)[NT], uint32_t yrow) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int cl0 = n * 16 + 4 * kg;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[n]), yd,
                                                   cl0 + 4 <= C ? yrow + 4u * cl0 : kOffOOB, 0, 0);
        }
        if (C % 4) {  // uniform
            // (the elements as separate values first, as in linear_split_kernel)
            const u32x4 pe = __builtin_bit_cast(u32x4, o[NT - 1]);
            const uint32_t e0 = pe.x, e1 = pe.y, e2 = pe.z;
            auto off = [&](int r) { return (ppart && pcl + r < C) ? yrow + 4u * (pcl + r) : kOffOOB; };
            __builtin_amdgcn_raw_buffer_store_b32(e0, yd, off(0), 0, 0);
            if (C % 4 >= 2) __builtin_amdgcn_raw_buffer_store_b32(e1, yd, off(1), 0, 0);
            if (C % 4 == 3) __builtin_amdgcn_raw_buffer_store_b32(e2, yd, off(2), 0, 0);
        }
    };
    auto flush = [&]() {
#pragma unroll
        for (int t = 0; t < PT; ++t)
            if (t < nheld) store_tile(held[t], hrow[t]);  // uniform
        nheld = 0;
    };
    // D[4 kg + r][j] = class n * 16 + 4 kg + r, row j
    stream<NT, NW, XT>(reinterpret_cast<char *>(sgr16), X, ldx, W, b, M, K, C,
                       [&](int tile, const f4 (&z)[NT]) {
        const int row = tile * 16 + j;  // rows past M: out-of-range offsets, dropped
        const uint32_t yrow = row < M ? (uint32_t)((int64_t)row * ldy * 4) : kOffOOB;
        if (nheld == PT) flush();
#pragma unroll
        for (int t = 0; t < PT; ++t)
            if (t == nheld) {  // uniform
#pragma unroll
                for (int n = 0; n < NT; ++n) held[t][n] = z[n];
                hrow[t] = yrow;
            }
        ++nheld;
    });
    flush();
}

// ---------------------------------------------------------------------------
// Weight backward: x16::dw_cols (x16_stream.h) as it stands.
template <int NT, typename XT>
__global__ __launch_bounds__(256) void xent_dw_cols_x16_kernel(
    const XT *__restrict__ X, int64_t ldx, const float *__restrict__ G, int ldg, int M, int K,
    int C, int n_cblk, int R, float *__restrict__ slab, float *__restrict__ db_slab) {
    x16::dw_cols<NT, XT>(X, ldx, G, ldg, M, K, C, n_cblk, R, slab, db_slab);
}

// ---------------------------------------------------------------------------
namespace {

// The layout both kernels need: even pitch, 4-B base, 31-bit byte offsets.
bool layout_ok(int64_t M, int64_t K, int64_t ldx, const void *X) {
    return M > 0 && K > 0 && ldx >= K && ldx % 2 == 0 && reinterpret_cast<uintptr_t>(X) % 4 == 0 &&
           M < INT32_MAX && K < INT32_MAX && M * ldx * 2 < INT32_MAX;
}

bool forward_covers(int64_t M, int64_t K, int64_t ldx, int64_t C, const void *X) {
    if (C <= 0 || !layout_ok(M, K, ldx, X)) return false;
    const int cc = (int)std::min<int64_t>(C, 64);  // the largest class block
    return K * cc < (int64_t(1) << 29) && x16::image_lds(K, cc) <= 160 * 1024;
}

bool backward_covers(int64_t M, int64_t K, int64_t ldx, int64_t C, const void *X) {
    return C > 0 && C <= 48 && layout_ok(M, K, ldx, X) && 32 * ldx * 2 < INT32_MAX;
}

inline int dw16_ranges(int64_t M) {
    return (int)std::min<int64_t>(x16::kDw16Ranges, std::max<int64_t>(1, (M + 31) / 32));
}

template <int NT, typename XT>
hipError_t launch_fwd16(const void *X, int64_t ldx, const float *W, const float *b, float *Y,
                        int64_t ldy, int M, int K, int C, hipStream_t s) {
    int blocks = 0;
    const hipError_t e = x16::persistent_grid(
        reinterpret_cast<const void *>(&linear_x16_kernel<NT, x16::kWaves, XT>), M, &blocks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((linear_x16_kernel<NT, x16::kWaves, XT>), dim3((unsigned)blocks),
                       dim3(64 * x16::kWaves), x16::image_lds(K, C), s, static_cast<const XT *>(X),
                       ldx, W, b, Y, ldy, M, K, C);
    return hipGetLastError();
}

template <typename XT>
hipError_t dispatch_fwd16(int nt, const void *X, int64_t ldx, const float *W, const float *b,
                          float *Y, int64_t ldy, int M, int K, int C, hipStream_t s) {
    switch (nt) {
        case 1: return launch_fwd16<1, XT>(X, ldx, W, b, Y, ldy, M, K, C, s);
        case 2: return launch_fwd16<2, XT>(X, ldx, W, b, Y, ldy, M, K, C, s);
        case 3: return launch_fwd16<3, XT>(X, ldx, W, b, Y, ldy, M, K, C, s);
        default: return launch_fwd16<4, XT>(X, ldx, W, b, Y, ldy, M, K, C, s);
    }
}

template <int NT, typename XT>
hipError_t launch_dw16(const void *X, int64_t ldx, const float *G, int ldg, int M, int K, int C,
                       float *slab, float *db_slab, hipStream_t s) {
    const int R = dw16_ranges(M);
    int n_cblk = 0;
    const int blocks = x16::dw_cols_blocks(K, R, &n_cblk);
    hipLaunchKernelGGL((xent_dw_cols_x16_kernel<NT, XT>), dim3(blocks), dim3(256), 0, s,
                       static_cast<const XT *>(X), ldx, G, ldg, M, K, C, n_cblk, R, slab, db_slab);
    return hipGetLastError();
}

template <typename XT>
hipError_t dispatch_dw16(int nt, const void *X, int64_t ldx, const float *G, int ldg, int M, int K,
                         int C, float *slab, float *db_slab, hipStream_t s) {
    switch (nt) {
        case 1: return launch_dw16<1, XT>(X, ldx, G, ldg, M, K, C, slab, db_slab, s);
        case 2: return launch_dw16<2, XT>(X, ldx, G, ldg, M, K, C, slab, db_slab, s);
        default: return launch_dw16<3, XT>(X, ldx, G, ldg, M, K, C, slab, db_slab, s);
    }
}

}  // namespace

const char *linear_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C, const void *X,
                                   int32_t x_dtype) {
    if (!dtype_ok(x_dtype) || !forward_covers(M, K, ldx, C, X)) return "none";
    return x_dtype == SGC_DTYPE_BF16
               ? "linear_x16_kernel (bf16 X streaming, v_mfma_f32_16x16x32_bf16 x 3 products)"
               : "linear_x16_kernel (fp16 X streaming, v_mfma_f32_16x16x32_bf16 x 5 products)";
}

int launch_linear_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                      float *Y, int64_t ldy, int64_t M, int64_t K, int64_t C, hipStream_t stream) {
    SGC_REQUIRE(dtype_ok(x_dtype), SGC_EINVAL,
                "linear_x16: x_dtype %d is neither SGC_DTYPE_BF16 nor SGC_DTYPE_F16", (int)x_dtype);
    SGC_REQUIRE(X && W && Y, SGC_EINVAL, "linear_x16: null pointer");
    SGC_REQUIRE(M >= 0 && K > 0 && C > 0 && ldx >= K && ldy >= C, SGC_EINVAL,
                "linear_x16: bad shape M=%lld K=%lld C=%lld ldx=%lld ldy=%lld", (long long)M,
                (long long)K, (long long)C, (long long)ldx, (long long)ldy);
    if (M == 0) return SGC_OK;
    SGC_REQUIRE(forward_covers(M, K, ldx, C, X) && M * ldy * 4 < INT32_MAX, SGC_EINVAL,
                "linear_x16: not covered (odd pitch %lld, 2-B-aligned base, a class block's W "
                "image past LDS at K=%lld C=%lld, or past 31-bit offsets at M=%lld)",
                (long long)ldx, (long long)K, (long long)C, (long long)M);
    for (int64_t c0 = 0; c0 < C; c0 += 64) {  // classes 64 at a time (NT <= 4 tiles of 16)
        const int cc = (int)std::min<int64_t>(64, C - c0);
        const int nt = (cc + 15) / 16;
        const float *Wc = W + c0 * K;
        const float *bc = b ? b + c0 : nullptr;
        const hipError_t e =
            x_dtype == SGC_DTYPE_BF16
                ? dispatch_fwd16<bf16_t>(nt, X, ldx, Wc, bc, Y + c0, ldy, (int)M, (int)K, cc, stream)
                : dispatch_fwd16<f16_t>(nt, X, ldx, Wc, bc, Y + c0, ldy, (int)M, (int)K, cc, stream);
        SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_x16 launch failed: %s", hipGetErrorString(e));
    }
    return SGC_OK;
}

// Launch B of the fused 16-bit step (xent16.hip): the plain kernel on G, the
// partials left for the caller's reduction.  Arguments checked by the caller.
int dw_cols_x16_ranges(int64_t M) { return dw16_ranges(M); }

hipError_t launch_dw_cols_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *G, int ldg,
                              int M, int K, int C, float *slab, float *db_slab, hipStream_t s) {
    const int nt = (C + 15) / 16;
    return x_dtype == SGC_DTYPE_BF16
               ? dispatch_dw16<bf16_t>(nt, X, ldx, G, ldg, M, K, C, slab, db_slab, s)
               : dispatch_dw16<f16_t>(nt, X, ldx, G, ldg, M, K, C, slab, db_slab, s);
}

const char *linear_backward_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                            const void *X, int32_t x_dtype) {
    if (!dtype_ok(x_dtype) || !backward_covers(M, K, ldx, C, X)) return "none";
    return x_dtype == SGC_DTYPE_BF16
               ? "xent_dw_cols_x16_kernel (bf16 X column blocks, v_mfma_f32_16x16x32_bf16 x 3 products)"
               : "xent_dw_cols_x16_kernel (fp16 X column blocks, v_mfma_f32_16x16x32_bf16 x 5 products)";
}

int64_t linear_backward_x16_workspace_bytes(int64_t M, int64_t K, int64_t C) {
    if (M <= 0 || K <= 0 || C <= 0) return 0;
    const int64_t C16 = (C + 15) / 16 * 16;
    const int64_t R = dw16_ranges(M);
    auto al = [](int64_t x) { return (x + 255) / 256 * 256; };
    return al(R * C16 * K * 4) + al(R * C16 * 4) + 512;
}

int linear_backward_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *dY, int64_t ldd,
                        int64_t M, int64_t K, int64_t C, float *dW, float *db, void *ws,
                        int64_t ws_bytes, hipStream_t s) {
    SGC_REQUIRE(dtype_ok(x_dtype), SGC_EINVAL,
                "linear_backward_x16: x_dtype %d is neither SGC_DTYPE_BF16 nor SGC_DTYPE_F16",
                (int)x_dtype);
    SGC_REQUIRE(X && dY && dW && ws, SGC_EINVAL, "linear_backward_x16: null pointer");
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && ldx >= K && ldd >= C, SGC_EINVAL,
                "linear_backward_x16: bad shape M=%lld K=%lld C=%lld", (long long)M, (long long)K,
                (long long)C);
    SGC_REQUIRE(backward_covers(M, K, ldx, C, X) && 32 * ldd * 4 < INT32_MAX, SGC_EINVAL,
                "linear_backward_x16: not covered (C=%lld > 48, odd pitch %lld, 2-B-aligned base, "
                "or past 31-bit offsets at M=%lld)",
                (long long)C, (long long)ldx, (long long)M);
    const int64_t need = linear_backward_x16_workspace_bytes(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "linear_backward_x16: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    const int NT = (int)((C + 15) / 16);
    const int C16 = NT * 16;
    const int R = dw16_ranges(M);
    auto al = [](int64_t x) { return (x + 255) / 256 * 256; };
    char *p = (char *)(((uintptr_t)ws + 255) & ~uintptr_t(255));
    float *slab = (float *)p;
    p += al((int64_t)R * C16 * K * 4);
    float *db_slab = db ? (float *)p : nullptr;
    hipError_t e = x_dtype == SGC_DTYPE_BF16
                       ? dispatch_dw16<bf16_t>(NT, X, ldx, dY, (int)ldd, (int)M, (int)K, (int)C, slab,
                                               db_slab, s)
                       : dispatch_dw16<f16_t>(NT, X, ldx, dY, (int)ldd, (int)M, (int)K, (int)C, slab,
                                              db_slab, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_backward_x16 launch failed: %s",
                hipGetErrorString(e));
    e = launch_reduce_dw_db(slab, R, (int)C, (int)K, C16, dW, db_slab, db, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_backward_x16 reduction failed: %s",
                hipGetErrorString(e));
    return SGC_OK;
}

}  // namespace sgc
