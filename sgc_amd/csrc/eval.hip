// eval.hip -- device-resident evaluation of the SGC classifier on gfx950: what
// the reference's test_regression computes from model(x) (citation.py:64-66
// accuracy, reddit.py:69-71 f1; TextSGC's eval_linear adds the mean loss),
// without the [M, C] logits matrix and without host code.
//
//   A  eval_fwd_kernel      logits of a 128-row block on fp32 MFMA (xent.hip's
//                           launch A: xwt_block_tile, the same row epilogue for
//                           max / exp / sum / (max - z_y) + log(sum)), then the
//                           row's argmax by eval.h's key across the 16-lane class
//                           group: pred [M] int64 and one loss partial per wave.
//                           No G, no logits, no dG sums are stored.
//      (16-bit X: eval_fwd_x16_kernel, eval16.hip, one loss partial per tile.)
//   B  eval_count_kernel    labels x predictions -> workgroup-local LDS integer
//                           counters (C x C and {counted, correct}), one partial
//                           table per workgroup in the workspace;
//   C  eval_finish_kernel   the partial tables summed in workgroup order ->
//                           confusion [C][C] int64, counts [2]; the loss partials
//                           in a fixed order (double) -> the mean loss.
// No atomics on global memory; integer sums are exact and the loss is summed
// in a fixed order, so every output is bitwise reproducible run to run.
//
// The counting is a launch of its own (B), not part of A's epilogue: the
// 16-bit kernel's W image leaves 5.4 KB of LDS at the Reddit shape (K = 602,
// C = 41) where a 41 x 41 counter table needs 6.7 KB.  B reads 16 bytes per
// row (0.9 MB at 55,334 rows against A's 67-133 MB) and both feature families
// share it.
//
// A label outside [0, C) leaves its row out of the matrix and the counts and
// makes the loss NaN; it never indexes the table.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "eval.h"
#include "gemm_tile.h"
#include "group16.h"
#include "internal.h"

namespace sgc {

namespace {

// (group16_max / group16_sum: group16.h)
__device__ __forceinline__ unsigned long long group16_key(unsigned long long k) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) k = key_max(k, __shfl_xor(k, m, 64));
    return k;
}

// ---- A: logits -> predictions, per-wave loss partials ----------------------
// xent_fwd_kernel's tile and row epilogue (xent.hip).  Lane (i, g) = (l & 15,
// l >> 4) holds classes 16 n + i of rows m0 + 16 t + 4 g + r; the 16 lanes of a
// group share a row.  pred (nullable): the row's class.  labels (nullable; the
// host passes them only when a loss is wanted): without them the softmax is
// skipped and loss_part is not written.
template <int V, int NT, int NB>
__global__ __launch_bounds__(256) void eval_fwd_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, const int64_t *__restrict__ labels, int M, int K, int C,
    int64_t *__restrict__ pred, double *__restrict__ loss_part) {
    __shared__ LdsTile<V, NT, NB> sm;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wave = blockIdx.x * 4 + w;
    const int i = lane & 15, g = lane >> 4;
    const int m_blk = blockIdx.x * kLdsBM;
    const int m0 = m_blk + w * 32;
    double wave_loss = 0.0;
    {
        f32x4 acc[2][NT];
        xwt_block_tile<V, NT, NB>(X, ldx, W, M, K, C, m_blk, sm, acc);
        float bias[NT];
        bool valid[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int c = n * 16 + i;
            valid[n] = c < C;
            bias[n] = (valid[n] && b) ? b[c] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + t * 16 + g * 4 + r;
                const bool row_ok = m < M;  // uniform per (t, r, lane group)
                float z[NT];
                float mx = -INFINITY;
                unsigned long long best = 0ull;  // no class: below every real one
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    z[n] = valid[n] ? acc[t][n][r] + bias[n] : -INFINITY;
                    mx = fmaxf(mx, z[n]);
                    if (valid[n]) best = key_max(best, argmax_key(z[n], n * 16 + i));
                }
                best = group16_key(best);
                if (pred && row_ok && i == 0) pred[m] = (int64_t)key_class(best);
                if (!labels) continue;  // (uniform for the grid)
                mx = group16_max(mx);
                float se = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n) se += valid[n] ? expf(z[n] - mx) : 0.f;
                se = group16_sum(se);
                // loss = (max - z_y) + log(sum), as xent_fwd_kernel
                const float ls = logf(se);
                const int64_t y = row_ok ? labels[m] : -1;
                float zy = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    if (n * 16 + i == y) zy = z[n];
                zy = group16_sum(zy);  // exactly one lane of the group holds z_y
                if (row_ok && i == 0)
                    wave_loss += (y >= 0 && y < C) ? (double)((mx - zy) + ls) : (double)NAN;
            }
    }
    if (!labels) return;
    double l = wave_loss;  // lanes i == 0 of each group
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (lane == 0) loss_part[wave] = l;
}

// ---- B: labels x predictions -> per-workgroup counter tables ----------------
// Workgroup blk counts rows [blk * rows_per, ...) into LDS (integer adds: the
// order does not matter) and stores its table: part[blk][C * C + 2], the last
// two entries {rows counted, rows correct}.  A row whose label or prediction
// lies outside [0, C) is left out.
constexpr int kCountRows = 2048;  // rows per counting workgroup, at least
constexpr int kCountBlocks = 256;  // counting workgroups, at most

__global__ __launch_bounds__(256) void eval_count_kernel(const int64_t *__restrict__ labels,
                                                         const int64_t *__restrict__ pred, int M,
                                                         int C, int rows_per,
                                                         int32_t *__restrict__ part) {
    __shared__ int tab[64 * 64 + 2];
    const int n = C * C;
    for (int e = threadIdx.x; e < n + 2; e += 256) tab[e] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rows_per;
    const int64_t r1 = std::min<int64_t>(M, r0 + rows_per);
    int counted = 0, correct = 0;
    for (int64_t m = r0 + threadIdx.x; m < r1; m += 256) {
        const int64_t y = labels[m], p = pred[m];
        if (y >= 0 && y < C && p >= 0 && p < C) {
            atomicAdd(&tab[(int)y * C + (int)p], 1);
            ++counted;
            correct += (p == y);
        }
    }
    atomicAdd(&tab[n], counted);
    atomicAdd(&tab[n + 1], correct);
    __syncthreads();
    int32_t *out = part + (int64_t)blockIdx.x * (n + 2);
    for (int e = threadIdx.x; e < n + 2; e += 256) out[e] = tab[e];
}

// ---- C: the fixed-order sums -------------------------------------------------
// Blocks [0, count_grid): thread e sums entry e of the n_blocks tables in
// workgroup order -> confusion[e] (e < C * C) or counts[e - C * C], each
// skipped when null.  The block after them (launched only for a loss): thread
// t sums partials t, t + 256, ... in order, then a fixed-shape LDS tree, in
// double (xent_reduce_small_kernel's order).
__global__ __launch_bounds__(256) void eval_finish_kernel(
    const int32_t *__restrict__ part, int n_blocks, int C, int count_grid,
    int64_t *__restrict__ confusion, int64_t *__restrict__ counts,
    const double *__restrict__ loss_part, int n_loss, double inv_m, float *__restrict__ loss) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int n = C * C;
    if ((int)blockIdx.x < count_grid) {
        const int e = (int)blockIdx.x * 256 + t;
        if (e < n + 2) {
            int64_t s = 0;
            for (int j = 0; j < n_blocks; ++j) s += part[(int64_t)j * (n + 2) + e];
            if (e < n) {
                if (confusion) confusion[e] = s;
            } else if (counts) {
                counts[e - n] = s;
            }
        }
        return;  // (uniform per block: no barrier below is reached)
    }
    double s = 0.0;
    for (int j = t; j < n_loss; j += 256) s += loss_part[j];
    red[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) *loss = (float)(red[0] * inv_m);
}

inline int count_blocks(int64_t M) {
    return (int)std::min<int64_t>(kCountBlocks, std::max<int64_t>(1, (M + kCountRows - 1) / kCountRows));
}

// Launch A: the (V, NT, NB) table of gemm_tile.h's dispatch_tile.
hipError_t launch_fwd(int V, int NT, const float *X, int64_t ldx, const float *W, const float *b,
                      const int64_t *labels, int M, int K, int C, int64_t *pred, double *loss_part,
                      hipStream_t s) {
    const int blocks = (M + kLdsBM - 1) / kLdsBM;
    dispatch_tile(V, NT, g_tile_buffers, [&](auto v, auto nt, auto nb) {
        hipLaunchKernelGGL(
            (eval_fwd_kernel<decltype(v)::value, decltype(nt)::value, decltype(nb)::value>),
            dim3(blocks), dim3(256), 0, s, X, ldx, W, b, labels, M, K, C, pred, loss_part);
    });
    return hipGetLastError();
}

// sgc_linear_xent_f32's limits, and every byte offset of X within 31 bits
bool covers_f32(int64_t M, int64_t K, int64_t ldx, int64_t C, const float *X) {
    return M > 0 && K > 0 && C > 0 && C <= 64 && ldx >= K && M < INT32_MAX && K < INT32_MAX &&
           reinterpret_cast<uintptr_t>(X) % 4 == 0 && M * ldx * 4 < (int64_t(1) << 31) &&
           block_tile_fits(ldx, K, C);
}

}  // namespace

// ---- what eval16.hip shares: the workspace and launches B and C --------------
// loss partials [n_loss] double | counter tables [count_blocks(M)][C * C + 2]
// int32 | predictions [M] int64 (used only when the caller passes no `pred`
// but wants the counts)
int64_t eval_workspace_bytes(int64_t M, int64_t C, int64_t n_loss) {
    return al256(n_loss * 8) + al256((int64_t)count_blocks(M) * (C * C + 2) * 4) + al256(M * 8) + 512;
}

EvalParts eval_carve(void *ws, int64_t M, int64_t C, int64_t n_loss) {
    EvalParts o;
    char *p = (char *)(((uintptr_t)ws + 255) & ~uintptr_t(255));
    o.loss_part = (double *)p;
    p += al256(n_loss * 8);
    o.count_part = (int32_t *)p;
    p += al256((int64_t)count_blocks(M) * (C * C + 2) * 4);
    o.pred = (int64_t *)p;
    return o;
}

// The pointer rules both entries share (nothing is dereferenced).
int eval_check_outputs(const char *what, const int64_t *labels, const int64_t *pred,
                       const int64_t *confusion, const int64_t *counts, const float *loss) {
    SGC_REQUIRE(labels || (!confusion && !counts && !loss), SGC_EINVAL,
                "%s: confusion, counts and loss need labels", what);
    SGC_REQUIRE(pred || confusion || counts || loss, SGC_EINVAL, "%s: no output requested", what);
    return SGC_OK;
}

int eval_count_finish(const int64_t *labels, const int64_t *pred, int64_t M, int64_t C,
                      const EvalParts &o, int n_loss, int64_t *confusion, int64_t *counts,
                      float *loss, hipStream_t s) {
    const bool count = confusion || counts;
    if (!count && !loss) return SGC_OK;
    const int nb = count_blocks(M);
    if (count) {
        const int rows_per = (int)((M + nb - 1) / nb);
        hipLaunchKernelGGL(eval_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, labels, pred,
                           (int)M, (int)C, rows_per, o.count_part);
        SGC_HIP_CHECK(hipGetLastError());
    }
    const int count_grid = count ? (int)((C * C + 2 + 255) / 256) : 0;
    hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)(count_grid + (loss ? 1 : 0))), dim3(256),
                       0, s, o.count_part, nb, (int)C, count_grid, confusion, counts, o.loss_part,
                       n_loss, 1.0 / (double)M, loss);
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

// ---- the fp32 entry ------------------------------------------------------------
const char *linear_eval_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C, const float *X) {
    if (!covers_f32(M, K, ldx, C, X)) return "none";
    return "eval_fwd_kernel (fp32 LDS tile, v_mfma_f32_16x16x4_f32, argmax + loss epilogue)";
}

static int64_t eval_f32_loss_parts(int64_t M) { return (M + kLdsBM - 1) / kLdsBM * 4; }

int64_t linear_eval_workspace_bytes(int64_t M, int64_t K, int64_t C) {
    if (!covers_f32(M, K, K, C, nullptr)) return 0;  // (the tightest layout)
    return eval_workspace_bytes(M, C, eval_f32_loss_parts(M));
}

int linear_eval_f32(const float *X, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, int64_t *pred,
                    int64_t *confusion, int64_t *counts, float *loss, void *ws, int64_t ws_bytes,
                    hipStream_t s) {
    SGC_REQUIRE(covers_f32(M, K, ldx, C, X), SGC_EINVAL,
                "linear_eval: not covered (M=%lld K=%lld C=%lld ldx=%lld: 1 <= C <= 64, ldx >= K, "
                "X 4-B aligned, M * ldx * 4 < 2^31)",
                (long long)M, (long long)K, (long long)C, (long long)ldx);
    if (const int rc = eval_check_outputs("linear_eval", labels, pred, confusion, counts, loss))
        return rc;
    SGC_REQUIRE(X && W && ws, SGC_EINVAL, "linear_eval: null pointer");
    const int n_loss = (int)eval_f32_loss_parts(M);
    const int64_t need = eval_workspace_bytes(M, C, n_loss);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "linear_eval: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    const EvalParts o = eval_carve(ws, M, C, n_loss);
    // the counts read the predictions back: the workspace's own when the caller wants none
    int64_t *p = pred ? pred : ((confusion || counts) ? o.pred : nullptr);
    // launch A reads the labels for the loss alone (the counts are launch B's): without a
    // loss it skips the softmax and writes no partials
    const int64_t *ya = loss ? labels : nullptr;
    const hipError_t e = launch_fwd(tile_vec(K, ldx, X, W), (int)((C + 15) / 16), X, ldx, W, b, ya,
                                    (int)M, (int)K, (int)C, p, o.loss_part, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_eval launch failed: %s", hipGetErrorString(e));
    return eval_count_finish(labels, p, M, C, o, n_loss, confusion, counts, loss, s);
}

}  // namespace sgc
