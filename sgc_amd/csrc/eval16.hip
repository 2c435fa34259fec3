// eval16.hip -- device-resident evaluation of the SGC classifier on 16-bit
// features (torch.bfloat16 / torch.float16 X; W and b fp32): launch A of
// eval.hip's chain on linear_x16_kernel's stream, X read once at 16 bits.
//
//   A  eval_fwd_x16_kernel  logits by the split-bf16 scheme on the persistent
//                           stream of linear16.hip (W's image built behind the
//                           first loads, the slot ring, every load issued on
//                           every path; one bf16 piece for bf16 X, two for
//                           fp16); each finished 16-row tile is followed at once
//                           by xent_fwd_x16_kernel's row epilogue without the G
//                           stores, plus the row's argmax by eval.h's key:
//                           pred [M] int64 and ONE LOSS PARTIAL PER TILE, a
//                           double indexed by tile number (the waves take tiles
//                           dynamically: a per-wave partial would differ run to
//                           run).
//   B, C                    eval.hip's counting and finishing launches.
//
// linear16.hip's text is included for namespace x16's helpers, the way
// xent16.hip includes it; the one kernel it then declares is never
// instantiated here.
//
// THE STREAM EXISTS THREE TIMES.  Everything in eval_fwd_x16_kernel from its
// first line down to `if (c == NC - 1)` -- the tile grab, the X descriptor and
// slot ring, W's image, the ror8 exchange, the ragged chunk and the MFMA block
// -- is a line-for-line copy of linear_x16_kernel (linear16.hip) and of
// xent_fwd_x16_kernel (xent16.hip); only the end of a tile differs.  A fix to
// the stream has to land in all three.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "eval.h"
#include "gemm_tile.h"
#include "internal.h"
#include "split_bf16.h"
#include "x16.h"

#define SGC_X16_KERNEL(name) name##_eval_unit_kernel
#define SGC_X16_STOP_PARAM const int64_t *__restrict__ stop,
#define SGC_X16_STOP_TEST \
    if (*stop != 0) return;
#define SGC_X16_STOP_PASS 1

namespace sgc {

namespace {
#include "linear16.hip"
}  // namespace

namespace {

// ---- A: logits -> predictions, per-tile loss partials -----------------------
// The stream is linear_x16_kernel's (see there); the end of a tile is
// xent_fwd_x16_kernel's.  Lane (j, kg) then holds row j of the tile and classes
// 16 n + 4 kg + r (n < NT, r < 4): the row's reductions -- the argmax key among
// them -- run over r and n in the lane, then across the four lanes j, j + 16,
// j + 32, j + 48 (xor 16, xor 32).  The predictions and the tile's partial go
// out through descriptors of the tile's own rows (rows past M lie outside them
// and are dropped).  pred and labels are nullable as in eval_fwd_kernel.
template <int NT, int NW, typename XT>
__global__ __launch_bounds__(64 * NW) void eval_fwd_x16_kernel(
    const XT *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, const int64_t *__restrict__ labels, int M, int K, int C,
    int64_t *__restrict__ pred, double *__restrict__ loss_tile) {
    using namespace x16;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) u32x4 sge16[];
    char *const lds = reinterpret_cast<char *>(sge16);
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, kg = lane >> 4;
    const int NC = (K + 63) / 64;         // double chunks per tile
    const int NH = half_chunks(K);        // half chunks of the image
    const int Cl = C - (NT - 1) * 16;     // classes of the last tile, 1..16
    const int cstride = chunk_bytes(NT, Cl);
    int *next = reinterpret_cast<int *>(lds + NH * cstride);
    if (threadIdx.x == 0) *next = 0;
    __syncthreads();
    const int n_tiles = (M + 15) >> 4;
    auto grab = [&]() -> int {  // the workgroup's next tile (block + grid * m), or -1
        int m = 0;
        if (lane == 0) m = atomicAdd(next, 1);
        m = __builtin_amdgcn_readfirstlane(m);
        const int t = (int)blockIdx.x + (int)gridDim.x * m;
        return t < n_tiles ? t : -1;
    };
    const auto xd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<XT *>(X), 0, (int)((int64_t)M * ldx * 2), 0x00020000);  // < 2^31, ldx even
    const uint32_t seg = 16u * (2 * kg + (j >> 3));
    const uint32_t pitch8 = (uint32_t)(8 * ldx * 2);
    int ltile = grab(), lc = 0;
    uint32_t lrow0 = 0, lrow1 = 0;
    auto rows_of = [&](int tile) {
        const int row = tile * 16 + (j & 7);
        lrow0 = (tile >= 0 && row < M) ? (uint32_t)((int64_t)row * ldx * 2) + seg : kOffOOB;
        lrow1 = (tile >= 0 && row + 8 < M) ? lrow0 + pitch8 : kOffOOB;
    };
    rows_of(ltile);
    constexpr int D = kDepth;
    u32x4 xa[D], xb[D];
    int stile[D], sc[D];
    auto load = [&](auto uc) {
        constexpr int u = decltype(uc)::value;
        stile[u] = ltile;
        sc[u] = lc;
        const uint32_t co = (uint32_t)lc * 128u;
        xa[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xd, lrow0 + co, 0, 0));
        xb[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xd, lrow1 + co, 0, 0));
        if (ltile >= 0 && ++lc == NC) {
            lc = 0;
            ltile = grab();
            rows_of(ltile);
        }
    };
    // the ring's first double chunks are in flight while W's image is built
    each_slot<0, D>(load);
    {
        // (linear_x16_kernel's image: granule (hc, kg) is k = 64 (hc >> 1) + 16 kg + 8 (hc & 1))
        const auto wd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0,
                                                          (int)((int64_t)C * K * 4), 0x00020000);
        const int full = (NT - 1) * 64;
        const int Gr = NH * 4;  // granules per class row
        constexpr int FU = 8;   // units per thread per round, loads all issued first
        for (int base = threadIdx.x; base < C * Gr; base += FU * 64 * NW) {
            f4 e[FU][2];
            int dsto[FU];
#pragma unroll
            for (int f = 0; f < FU; ++f) {
                const int idx = base + f * 64 * NW;
                const bool in = idx < C * Gr;
                const int r = in ? idx / Gr : 0, g = in ? idx - r * Gr : 0;
                const int hc = g >> 2, kk = g & 3, n = r >> 4, jj = r & 15;
                const int k0 = 64 * (hc >> 1) + 16 * kk + 8 * (hc & 1);
                const int w = n < NT - 1 ? n * 64 + jj + 16 * kk : full + kk * Cl + jj;
                dsto[f] = in ? hc * cstride + w * 48 : -1;
                const uint32_t off = k0 < K ? (uint32_t)(r * K + k0) * 4u : kOffOOB;
                e[f][0] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(wd, off, 0, 0));
                e[f][1] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(wd, off + 16, 0, 0));
                if (k0 + 8 > K) {  // the row's last granule: k >= K is the next row
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (k0 + q >= K) e[f][q >> 2][q & 3] = 0.0f;
                }
            }
#pragma unroll
            for (int f = 0; f < FU; ++f) {
                uint32_t h[4], m[4], l[4];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    split3(e[f][p >> 1][2 * (p & 1)], e[f][p >> 1][2 * (p & 1) + 1], h[p], m[p], l[p]);
                if (dsto[f] >= 0) {
                    char *dst = lds + dsto[f];
                    *reinterpret_cast<u32x4 *>(dst) = u32x4{h[0], h[1], h[2], h[3]};
                    *reinterpret_cast<u32x4 *>(dst + 16) = u32x4{m[0], m[1], m[2], m[3]};
                    *reinterpret_cast<u32x4 *>(dst + 32) = u32x4{l[0], l[1], l[2], l[3]};
                }
            }
        }
        // the zero granule of each half chunk's last class tile (its lanes past Cl)
        for (int c = threadIdx.x; c < NH; c += 64 * NW) {
            char *dst = lds + c * cstride + (full + 4 * Cl) * 48;
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x4 *>(dst + 16 * p) = u32x4{0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();
    const uint32_t bfull = (uint32_t)lane * 48u;
    const uint32_t blast = (NT - 1) * 3072u + 48u * (uint32_t)(j < Cl ? kg * Cl + j : 4 * Cl);
    f4 bias[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cl = n * 16 + 4 * kg + r;
            bias[n][r] = (b && cl < C) ? b[cl] : 0.0f;
        }
    // the loss partials: one double per tile (n_tiles * 8 < 2^31); an empty
    // range without labels
    const auto ld = __builtin_amdgcn_make_buffer_rsrc(loss_tile, 0, labels ? n_tiles * 8 : 0,
                                                      0x00020000);
    f32x4 accH[NT], accL[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) accH[n] = accL[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool low = j < 8;
    auto step = [&](auto uc) -> bool {  // false: the stream is done (uniform)
        constexpr int u = decltype(uc)::value;
        const int tile = stile[u], c = sc[u];
        if (tile < 0) return false;
        const u32x4 A = xa[u], B = xb[u];
        uint32_t v[8];  // dword d: k = 64c + 16kg + 2d, + 1 of row j
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t t = ror8(low ? B[e] : A[e]);
            v[e] = low ? A[e] : t;
            v[4 + e] = low ? t : B[e];
        }
        load(uc);  // the double chunk D ahead into the slot just consumed
        if ((c + 1) * 64 > K) {  // the ragged last double chunk (uniform)
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int k = c * 64 + 16 * kg + 2 * d;
                v[d] = k >= K ? 0u : k + 1 >= K ? (v[d] & 0xffffu) : v[d];
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int hc = 2 * c + q;
            if (hc >= NH) continue;  // wholly past K (uniform): no image, no MFMAs
            u32x4 bw[NT][3];
            {
                const uint32_t coff = (uint32_t)hc * (uint32_t)cstride;
                const char *af = lds + bfull + coff;
                const char *al = lds + blast + coff;
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        bw[n][p] = *reinterpret_cast<const u32x4 *>(
                            (n < NT - 1 ? af + n * 3072 : al) + 16 * p);
            }
            uint32_t ah[4], am[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) pieces16<XT>(v[4 * q + p], ah[p], am[p]);
            const bf16x8_t Xh = __builtin_bit_cast(bf16x8_t, u32x4{ah[0], ah[1], ah[2], ah[3]});
            auto wb = [&](int n, int p) { return __builtin_bit_cast(bf16x8_t, bw[n][p]); };
#pragma unroll
            for (int n = 0; n < NT; ++n)
                accH[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 0), Xh, accH[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < NT; ++n)
                accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 1), Xh, accL[n], 0, 0, 0);
            if constexpr (__is_same(XT, f16_t)) {
                const bf16x8_t Xm = __builtin_bit_cast(bf16x8_t, u32x4{am[0], am[1], am[2], am[3]});
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 0), Xm, accL[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 2), Xh, accL[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 1), Xm, accL[n], 0, 0, 0);
            } else {
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 2), Xh, accL[n], 0, 0, 0);
            }
        }
        if (c == NC - 1) {  // tile done: D[4 kg + r][j] = class n * 16 + 4 kg + r, row j
            const int row0 = tile * 16;
            const int rows = min(16, M - row0);  // uniform, >= 1
            const bool row_ok = j < rows;
            f4 z[NT];
            float mx = -INFINITY;
            unsigned long long best = 0ull;  // no class: below every real one
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                z[n] = accH[n] + accL[n] + bias[n];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cl = n * 16 + 4 * kg + r;
                    if (cl >= C)
                        z[n][r] = -INFINITY;
                    else
                        best = key_max(best, argmax_key(z[n][r], cl));
                    mx = fmaxf(mx, z[n][r]);
                }
                accH[n] = accL[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            best = key_max(best, __shfl_xor(best, 16, 64));
            best = key_max(best, __shfl_xor(best, 32, 64));
            if (pred) {  // (uniform) lanes kg == 0: row j of the tile's `rows` rows
                const auto pd = __builtin_amdgcn_make_buffer_rsrc(pred + row0, 0, rows * 8, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)key_class(best), 0u}, pd,
                                                      kg == 0 ? (uint32_t)j * 8u : kOffOOB, 0, 0);
            }
            if (labels) {  // (uniform)
                // the tile's labels, uniform addresses; lane (j, .) keeps row j's
                int y = -1;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t yi = labels[row0 + min(i, rows - 1)];
                    const int ys = (yi >= 0 && yi < C) ? (int)yi : -1;
                    y = (j == i) ? ys : y;
                }
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                float se = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        se += n * 16 + 4 * kg + r < C ? expf(z[n][r] - mx) : 0.f;
                se += __shfl_xor(se, 16, 64);
                se += __shfl_xor(se, 32, 64);
                // loss = (max - z_y) + log(sum), as xent_fwd_kernel
                const float ls = logf(se);
                float zy = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n * 16 + 4 * kg + r == y) zy = z[n][r];
                zy += __shfl_xor(zy, 16, 64);  // exactly one lane of the four holds z_y
                zy += __shfl_xor(zy, 32, 64);
                // a label outside [0, C): NaN, as sgc_cross_entropy_f32
                double l = row_ok ? (y >= 0 ? (double)((mx - zy) + ls) : (double)NAN) : 0.0;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) l += __shfl_xor(l, o, 64);  // the 16 rows, a fixed tree
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, l), ld,
                                                      lane == 0 ? (uint32_t)tile * 8u : kOffOOB, 0, 0);
            }
        }
        return true;
    };
    for (;;) {
        if (!run_slots<0, D>(step)) break;
    }
}

bool dtype_ok(int32_t x_dtype) { return x_dtype == SGC_DTYPE_BF16 || x_dtype == SGC_DTYPE_F16; }

inline size_t fwd_lds(int K, int C) {
    const int NT = (C + 15) / 16;
    return (size_t)x16::half_chunks(K) * x16::chunk_bytes(NT, C - (NT - 1) * 16) + 16;
}

template <int NT, typename XT>
hipError_t launch_fwd(const void *X, int64_t ldx, const float *W, const float *b,
                      const int64_t *labels, int M, int K, int C, int64_t *pred, double *loss_tile,
                      hipStream_t s) {
    int cus = 0;
    hipError_t e = persistent_setup(
        reinterpret_cast<const void *>(&eval_fwd_x16_kernel<NT, x16::kWaves, XT>), &cus);
    if (e != hipSuccess) return e;
    const int tiles = (M + 15) / 16;
    const int blocks = std::max(1, std::min(cus, tiles));
    hipLaunchKernelGGL((eval_fwd_x16_kernel<NT, x16::kWaves, XT>), dim3((unsigned)blocks),
                       dim3(64 * x16::kWaves), fwd_lds(K, C), s, static_cast<const XT *>(X), ldx, W,
                       b, labels, M, K, C, pred, loss_tile);
    return hipGetLastError();
}

template <typename XT>
hipError_t dispatch_fwd(int nt, const void *X, int64_t ldx, const float *W, const float *b,
                        const int64_t *labels, int M, int K, int C, int64_t *pred,
                        double *loss_tile, hipStream_t s) {
    switch (nt) {
        case 1: return launch_fwd<1, XT>(X, ldx, W, b, labels, M, K, C, pred, loss_tile, s);
        case 2: return launch_fwd<2, XT>(X, ldx, W, b, labels, M, K, C, pred, loss_tile, s);
        case 3: return launch_fwd<3, XT>(X, ldx, W, b, labels, M, K, C, pred, loss_tile, s);
        default: return launch_fwd<4, XT>(X, ldx, W, b, labels, M, K, C, pred, loss_tile, s);
    }
}

}  // namespace

// What sgc_linear_x16_kernel_name covers, in one class block.
const char *linear_eval_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                        const void *X, int32_t x_dtype) {
    if (C > 64 || std::strcmp(linear_x16_kernel_name(M, K, ldx, C, X, x_dtype), "none") == 0)
        return "none";
    return x_dtype == SGC_DTYPE_BF16
               ? "eval_fwd_x16_kernel (bf16 X streaming, v_mfma_f32_16x16x32_bf16 x 3 products, "
                 "argmax + loss epilogue)"
               : "eval_fwd_x16_kernel (fp16 X streaming, v_mfma_f32_16x16x32_bf16 x 5 products, "
                 "argmax + loss epilogue)";
}

int64_t linear_eval_x16_workspace_bytes(int64_t M, int64_t K, int64_t C) {
    // every covered shape at its tightest layout (ldx = K rounded up to even, an aligned base)
    if (std::strcmp(linear_eval_x16_kernel_name(M, K, (K + 1) / 2 * 2, C, nullptr, SGC_DTYPE_BF16),
                    "none") == 0)
        return 0;
    return eval_workspace_bytes(M, C, (M + 15) / 16);
}

int linear_eval_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, int64_t *pred,
                    int64_t *confusion, int64_t *counts, float *loss, void *ws, int64_t ws_bytes,
                    hipStream_t s) {
    SGC_REQUIRE(dtype_ok(x_dtype), SGC_EINVAL,
                "linear_eval_x16: x_dtype %d is neither SGC_DTYPE_BF16 nor SGC_DTYPE_F16",
                (int)x_dtype);
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && ldx >= K, SGC_EINVAL,
                "linear_eval_x16: bad shape M=%lld K=%lld C=%lld ldx=%lld (ldx >= K)", (long long)M,
                (long long)K, (long long)C, (long long)ldx);
    SGC_REQUIRE(std::strcmp(linear_eval_x16_kernel_name(M, K, ldx, C, X, x_dtype), "none") != 0,
                SGC_EINVAL,
                "linear_eval_x16: not covered (C=%lld > 64, odd pitch %lld, 2-B-aligned base, W's "
                "image past LDS at K=%lld, or past 31-bit offsets at M=%lld)",
                (long long)C, (long long)ldx, (long long)K, (long long)M);
    if (const int rc = eval_check_outputs("linear_eval_x16", labels, pred, confusion, counts, loss))
        return rc;
    SGC_REQUIRE(X && W && ws, SGC_EINVAL, "linear_eval_x16: null pointer");
    const int n_tiles = (int)((M + 15) / 16);
    const int64_t need = eval_workspace_bytes(M, C, n_tiles);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "linear_eval_x16: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    const EvalParts o = eval_carve(ws, M, C, n_tiles);
    // the counts read the predictions back: the workspace's own when the caller wants none
    int64_t *p = pred ? pred : ((confusion || counts) ? o.pred : nullptr);
    const int nt = (int)((C + 15) / 16);
    const int64_t *ya = loss ? labels : nullptr;  // launch A reads them for the loss alone
    const hipError_t e =
        x_dtype == SGC_DTYPE_BF16
            ? dispatch_fwd<bf16_t>(nt, X, ldx, W, b, ya, (int)M, (int)K, (int)C, p, o.loss_part, s)
            : dispatch_fwd<f16_t>(nt, X, ldx, W, b, ya, (int)M, (int)K, (int)C, p, o.loss_part, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_eval_x16 launch failed: %s",
                hipGetErrorString(e));
    return eval_count_finish(labels, p, M, C, o, n_tiles, confusion, counts, loss, s);
}

}  // namespace sgc
