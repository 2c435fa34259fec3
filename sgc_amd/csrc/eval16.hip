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
#include <algorithm>
#include <cmath>
#include <cstring>

#include "eval.h"
#include "x16_stream.h"

namespace sgc {

namespace {

// ---- A: logits -> predictions, per-tile loss partials -----------------------
// x16::stream (x16_stream.h); the end of a tile is xent_fwd_x16_kernel's.  Lane
// (j, kg) then holds row j of the tile and classes 16 n + 4 kg + r (n < NT,
// r < 4): the row's reductions -- the argmax key among them -- run over r and n
// in the lane, then across the four lanes j, j + 16, j + 32, j + 48 (xor 16,
// xor 32).  The predictions and the tile's partial go out through descriptors
// of the tile's own rows (rows past M lie outside them and are dropped).  pred
// and labels are nullable as in eval_fwd_kernel.
template <int NT, int NW, typename XT>
__global__ __launch_bounds__(64 * NW) void eval_fwd_x16_kernel(
    const XT *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, const int64_t *__restrict__ labels, int M, int K, int C,
    int64_t *__restrict__ pred, double *__restrict__ loss_tile) {
    using namespace x16;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) u32x4 sge16[];
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, kg = lane >> 4;
    // the loss partials: one double per tile (n_tiles * 8 < 2^31); an empty
    // range without labels
    const auto ld = __builtin_amdgcn_make_buffer_rsrc(loss_tile, 0, labels ? ((M + 15) >> 4) * 8 : 0,
                                                      0x00020000);
    stream<NT, NW, XT>(reinterpret_cast<char *>(sge16), X, ldx, W, b, M, K, C,
                       [&](int tile, f4 (&z)[NT]) {
        const int row0 = tile * 16;
        const int rows = min(16, M - row0);  // uniform, >= 1
        const bool row_ok = j < rows;
        float mx = -INFINITY;
        unsigned long long best = 0ull;  // no class: below every real one
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cl = n * 16 + 4 * kg + r;
                if (cl >= C)
                    z[n][r] = -INFINITY;
                else
                    best = key_max(best, argmax_key(z[n][r], cl));
                mx = fmaxf(mx, z[n][r]);
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
    });
}

template <int NT, typename XT>
hipError_t launch_fwd(const void *X, int64_t ldx, const float *W, const float *b,
                      const int64_t *labels, int M, int K, int C, int64_t *pred, double *loss_tile,
                      hipStream_t s) {
    int blocks = 0;
    const hipError_t e = x16::persistent_grid(
        reinterpret_cast<const void *>(&eval_fwd_x16_kernel<NT, x16::kWaves, XT>), M, &blocks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((eval_fwd_x16_kernel<NT, x16::kWaves, XT>), dim3((unsigned)blocks),
                       dim3(64 * x16::kWaves), x16::image_lds(K, C), s, static_cast<const XT *>(X),
                       ldx, W, b, labels, M, K, C, pred, loss_tile);
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
