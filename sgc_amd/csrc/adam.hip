// adam.hip -- device-resident Adam for the citation driver's training loop
// (reference citation.py:41-50: 100 epochs of zero_grad, model(x),
// F.cross_entropy, backward, optim.Adam.step).
//
//   sgc_adam_step_f32    one launch updates up to 16 parameter tensors, their
//                        exp_avg and exp_avg_sq in place (adam_update.h: the
//                        element update and its operation order);
//   sgc_train_adam_f32   the whole loop: `epochs` fused epochs enqueued on one
//                        stream by one host call, on one of two schedules.
//
// General schedule (any M; xent.hip): launches A and B of the fused classifier
// step, then xent_reduce_adam_kernel -- three launches per epoch.
//
// Small schedule (M <= kSmallMaxM; this file): the citation train sets are
// 60-140 rows x 500-3703 features x 3-7 classes, where the Reddit-shaped
// kernels put the forward on two workgroups.  Here both launches of an epoch
// run one workgroup per 64-column block of K (8, 23 and 58 workgroups at
// Pubmed, Cora and Citeseer):
//   1  adam_small_logits_kernel   P[block][M][C16] = X[:, block] W[:, block]^T,
//                                 k ascending, one fmaf per product; block 0
//                                 also copies b into the workspace;
//   2  adam_small_update_kernel   every workgroup sums the partial logits over
//                                 the blocks in ascending order, adds the bias
//                                 copy, forms the row softmax, the loss terms
//                                 (max - z_y) + log(sum) and G = (softmax -
//                                 onehot) / M in LDS, then
//                                 dW[:, block] = G^T X[:, block] over all M
//                                 rows (m ascending, one fmaf per product) and
//                                 the Adam update of W[:, block]; workgroup 0
//                                 also finishes db, updates b and writes the
//                                 epoch's loss.
// Launch 2 writes the block of W that launch 1 of the next epoch reads, and no
// workgroup of launch 2 reads another block's W: the partial logits carry all
// the cross-block information, so the in-place update is race-free.  The bias
// is the one value every workgroup of launch 2 needs and workgroup 0 updates:
// launch 2 therefore reads the copy launch 1 made, never b itself.
// X is read with 4-B loads only (any K, any ldx >= K, a 4-B aligned base), and
// never past column K of a row.  No atomics; every sum has a fixed order.
//
//   sgc_train_adam_sweep_f32   B models on the same X and labels (the weight-
//                        decay search of the reference's tuning.py): the two
//                        launches above on a K-block x model grid
//                        (adam_sweep_logits_kernel, adam_sweep_update_kernel).
// Both pairs of kernels run the same __device__ bodies (small_logits_body,
// small_update_body); the batched pair hands them model blockIdx.y's slices of
// W, b and the moments, its own partial-logit area and bias copy in the
// workspace, and its own decay, read from the device table.  A workgroup of
// model i reads and writes model i's slices and area only, so the argument
// above holds model by model: across models nothing is shared but X and the
// labels, which no launch writes.  Each model's result is bit-identical to a
// single-model call.
#include <algorithm>
#include <cmath>

#include "adam_update.h"
#include "internal.h"

namespace sgc {


// sgc_set_tuning("adam_kernel"): 0 auto, 1 general, 2 small (where eligible).
int g_adam_kernel = 0;
// The schedule the last sgc_train_adam_f32 call ran (1 / 2; 0: none yet).
int g_adam_kernel_last = 0;
// What the last sgc_train_adam_sweep_f32 call ran: 2 the batched small
// schedule, 1 the general schedule model by model, 0 none yet.
int g_adam_sweep_last = 0;
// sgc_set_tuning("adam_sweep_form"): the batched launch 2 -- 0 auto, 1 fused (one
// launch), 2 split (softmax per model, then dW over K-block x model); and the
// form the last batched call ran (1 / 2; 0: none yet).
int g_adam_sweep_form = 0;
int g_adam_sweep_form_last = 0;
constexpr int kSweepMaxModels = 4096;

AdamCoef adam_coef(int64_t step, double lr, double beta1, double beta2, double eps,
                   double weight_decay) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamCoef c;
    c.wd = (float)weight_decay;
    c.omb1 = (float)(1.0 - beta1);
    c.b2 = (float)beta2;
    c.omb2 = (float)(1.0 - beta2);
    c.bc2_sqrt = (float)std::sqrt(bc2);
    c.eps = (float)eps;
    c.step_size = (float)(lr / bc1);
    return c;
}

namespace {

constexpr int kMaxTensors = 16;
constexpr int kStepPerBlock = 1024;  // elements per workgroup: 4 per thread

struct AdamTensors {
    float *p[kMaxTensors];
    const float *g[kMaxTensors];
    float *m[kMaxTensors];
    float *v[kMaxTensors];
    int64_t n[kMaxTensors];
    int32_t blk0[kMaxTensors + 1];  // first workgroup of each tensor (a skipped tensor has none)
};

__global__ __launch_bounds__(256) void adam_step_kernel(AdamTensors T, AdamCoef coef) {
    const int blk = blockIdx.x;
    int ti = 0;
#pragma unroll
    for (int i = 1; i < kMaxTensors; ++i)
        if (blk >= T.blk0[i]) ti = i;
    // (tensors without workgroups share their successor's blk0: the last i
    // with blk0[i] <= blk is the one that owns blk)
    const int64_t n = T.n[ti];
    float *p = T.p[ti], *m = T.m[ti], *v = T.v[ti];
    const float *g = T.g[ti];
    const int64_t base = (int64_t)(blk - T.blk0[ti]) * kStepPerBlock + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kStepPerBlock / 256; ++u) {
        const int64_t i = base + u * 256;
        if (i < n) {
            float pv = p[i], mv = m[i], vv = v[i];
            adam_update(pv, mv, vv, g[i], coef);
            p[i] = pv;
            m[i] = mv;
            v[i] = vv;
        }
    }
}

// ---- small schedule -----------------------------------------------------------
constexpr int kSmallBK = 64;  // columns of K per workgroup
// LDS of launch 2: G [M][C16 + 1] (the pad column holds the row's loss term),
// the X tile [M][64], and 2 KB of reduction scratch.  At C16 = 64 that is
// 516 B per row: (160 KB - 2 KB) / 516 B = 313 rows.
constexpr int kSmallScratch = 2048;
constexpr int kSmallMaxM = 313;
constexpr int64_t kLdsMax = 160 * 1024;
static_assert((int64_t)kSmallMaxM * (64 + 1 + kSmallBK) * 4 + kSmallScratch <= kLdsMax &&
                  (int64_t)(kSmallMaxM + 1) * (64 + 1 + kSmallBK) * 4 + kSmallScratch > kLdsMax,
              "kSmallMaxM is what 160 KB of LDS hold at 64 classes");

inline int64_t small_lds1(int64_t M, int64_t C16) { return (kSmallBK * C16 + M * (kSmallBK + 1)) * 4; }
inline int64_t small_lds2(int64_t M, int64_t C16) {
    return kSmallScratch + (M * (C16 + 1) + M * kSmallBK) * 4;
}

// rows x 64 columns [k0, k0 + 64) of X into LDS (row stride ld), zeros past K
__device__ __forceinline__ void load_x_tile(const float *__restrict__ X, int64_t ldx, int M, int K,
                                            int k0, float *xs, int ld) {
    const int k = threadIdx.x & 63;
    const bool ok = k0 + k < K;
    // 16 rows' loads in flight per thread: the workgroup is alone on its CU,
    // so nothing else hides a load's latency (one load at a time cost a
    // latency per four rows of M, eight at a time still 4 us at M = 140)
    for (int m0 = threadIdx.x >> 6; m0 < M; m0 += 64) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int m = m0 + 4 * u;
            v[u] = (ok && m < M) ? X[(int64_t)m * ldx + k0 + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int m = m0 + 4 * u;
            if (m < M) xs[m * ld + k] = v[u];
        }
    }
}

// Launch 1 of one model: K-block `blk` of the model whose W, b, P and bias copy
// are given (the single-model kernel passes its arguments, the batched one
// the slices of model blockIdx.y).
__device__ __forceinline__ void small_logits_body(
    const unsigned blk, const float *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, int M, int K, int C, int C16, float *__restrict__ P,
    float *__restrict__ bias_copy, float *lds1) {
    float *wt = lds1;                  // [64][C16]: W's block, transposed
    float *xs = lds1 + kSmallBK * C16;  // [M][65]
    const int k0 = blk * kSmallBK;
    {
        const int k = threadIdx.x & 63;
        const bool ok = k0 + k < K;
        for (int c0 = threadIdx.x >> 6; c0 < C16; c0 += 16) {  // (C16 is a multiple of 16)
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = (ok && c0 + 4 * u < C) ? W[(int64_t)(c0 + 4 * u) * K + k0 + k] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) wt[k * C16 + c0 + 4 * u] = v[u];
        }
    }
    load_x_tile(X, ldx, M, K, k0, xs, kSmallBK + 1);
    if (blk == 0 && (int)threadIdx.x < C16)
        bias_copy[threadIdx.x] = (b && (int)threadIdx.x < C) ? b[threadIdx.x] : 0.f;
    __syncthreads();
    // a task: row m, classes 4 c4 .. 4 c4 + 3
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int q4 = C16 >> 2;
    float *out = P + (int64_t)blk * M * C16;
    for (int o = threadIdx.x; o < M * q4; o += 256) {
        const int m = o / q4, c4 = o - m * q4;
        const float *xr = xs + m * (kSmallBK + 1);
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int k = 0; k < kSmallBK; ++k) {
            const float x = xr[k];
            const f4 w = *reinterpret_cast<const f4 *>(wt + k * C16 + 4 * c4);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(x, w[q], acc[q]);
        }
        *reinterpret_cast<f4 *>(out + (int64_t)m * C16 + 4 * c4) = acc;
    }
}

__global__ __launch_bounds__(256) void adam_small_logits_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, int M, int K, int C, int C16, float *__restrict__ P,
    float *__restrict__ bias_copy) {
    extern __shared__ __attribute__((aligned(16))) float lds1[];
    small_logits_body(blockIdx.x, X, ldx, W, b, M, K, C, C16, P, bias_copy, lds1);
}

// The batched grid: K-block x model.  Model i = blockIdx.y owns W + i w_stride,
// b + i C and the workspace area ws + i ws_stride floats (its bias copy, then
// its partial logits at kSweepBias floats).
constexpr int kSweepBias = 64;  // floats ahead of a model's P: its bias copy (256 B)
__global__ __launch_bounds__(256) void adam_sweep_logits_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, int M, int K, int C, int C16, float *__restrict__ ws,
    int64_t w_stride, int64_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) float sweep_lds1[];
    const int64_t i = blockIdx.y;
    float *area = ws + i * ws_stride;
    small_logits_body(blockIdx.x, X, ldx, W + i * w_stride, b ? b + i * C : nullptr, M, K, C, C16,
                      area + kSweepBias, area, sweep_lds1);
}

// Launch 2 of one model, in three parts that the batched split form runs in
// two launches (a workgroup per model for the first and the last, then the
// K-block x model grid for the second).
// Part 1: z = partial logits summed over the blocks + bias, the row softmax,
// G = (softmax - onehot) / M and the rows' loss terms, into gs [M][C16 + 1].
template <int NT>
__device__ __forceinline__ void small_softmax_part(
    const int64_t *__restrict__ labels, int M, int C, int n_blk, const float *__restrict__ P,
    const float *__restrict__ bias_copy, float inv_m, float *gs) {
    constexpr int C16 = NT * 16, LDG = C16 + 1;
    const int t = threadIdx.x;
    // z = (sum of the partial logits, blocks ascending) + bias
    // (four elements per thread at a time, 16 blocks each: 64 loads in
    // flight; an element past M * C or a block past n_blk adds 0, after the
    // real ones, so every sum is the plain ascending one)
    const int64_t pstride = (int64_t)M * C16;
    const int n_el = M * C;
    for (int o0 = t; o0 < n_el; o0 += 4 * 256) {
        const float *p[4];
        float s[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int o = min(o0 + 256 * a, n_el - 1);
            const int m = o / C;
            p[a] = P + (int64_t)m * C16 + (o - m * C);
            s[a] = 0.f;
        }
        for (int j = 0; j < n_blk; j += 16) {
            float v[4][16];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    v[a][u] = j + u < n_blk ? p[a][(int64_t)(j + u) * pstride] : 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int u = 0; u < 16; ++u) s[a] += v[a][u];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int o = o0 + 256 * a;
            if (o < n_el) {
                const int m = o / C, c = o - m * C;
                gs[m * LDG + c] = s[a] + bias_copy[c];
            }
        }
    }
    __syncthreads();
    // row softmax, loss term and G = (softmax - onehot) / M: one thread per row
    for (int m = t; m < M; m += 256) {
        float *z = gs + m * LDG;
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
        const int64_t y = labels[m];
        const float zy = (y >= 0 && y < C) ? z[y] : NAN;  // (labels are the caller's contract)
        float se = 0.f;
        for (int c = 0; c < C; ++c) {
            const float ez = expf(z[c] - mx);
            z[c] = ez;
            se += ez;
        }
        const float ls = logf(se);
        for (int c = 0; c < C; ++c) z[c] = (z[c] / se - (c == y ? 1.f : 0.f)) * inv_m;
        z[C16] = (mx - zy) + ls;
    }
    __syncthreads();
}

// Part 2: dW of K-block k0 / 64 from gs and the X tile xs [M][64], then the
// Adam update of that block of W.
template <int NT>
__device__ __forceinline__ void small_dw_part(
    const int k0, float *__restrict__ W, float *__restrict__ mW, float *__restrict__ vW, int M,
    int K, int C, const float *gs, const float *xs, const AdamCoef &coef) {
    constexpr int C16 = NT * 16, LDG = C16 + 1, NQ = C16 / 4;
    const int t = threadIdx.x;
    // dW[c][k0 + k] = sum_m G[m][c] X[m][k0 + k]: wave w owns classes w, w + 4, ...
    {
        const int w = __builtin_amdgcn_readfirstlane(t >> 6), k = t & 63;
        float acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
#pragma unroll 4
        for (int m = 0; m < M; ++m) {
            const float x = xs[m * kSmallBK + k];
            const float *gr = gs + m * LDG + w;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (w + 4 * q < C) acc[q] = fmaf(gr[4 * q], x, acc[q]);
        }
        if (k0 + k < K) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = w + 4 * q;
                if (c < C) {
                    const int64_t e = (int64_t)c * K + k0 + k;
                    float pw = W[e], m1 = mW[e], v1 = vW[e];
                    adam_update(pw, m1, v1, acc[q], coef);
                    W[e] = pw;
                    mW[e] = m1;
                    vW[e] = v1;
                }
            }
        }
    }
}

// Part 3 (one workgroup per model): db from gs, the update of b, the loss.
template <int NT>
__device__ __forceinline__ void small_bias_part(
    float *__restrict__ b, float *__restrict__ mb, float *__restrict__ vb, int M, int C,
    const float *gs, float *scratch, double inv_m_d, const AdamCoef &coef,
    float *__restrict__ loss_out) {
    constexpr int C16 = NT * 16, LDG = C16 + 1;
    double *lossp = reinterpret_cast<double *>(scratch);  // [1]
    float *dbp = scratch + 8;                              // [4][64]
    const int t = threadIdx.x;
    // db[c]: four interleaved partial sums over the rows, then in order
    {
        const int c = t & 63, part = t >> 6;
        float f = 0.f;
        if (c < C)
            for (int m = part; m < M; m += 4) f += gs[m * LDG + c];
        dbp[part * 64 + c] = f;
    }
    if (t < 64 && loss_out) {  // the loss: lane l sums rows l, l + 64, ..., then a xor tree
        double s = 0.0;
        for (int m = t; m < M; m += 64) s += (double)gs[m * LDG + C16];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (t == 0) *lossp = s;
    }
    __syncthreads();
    if (t == 0 && loss_out) *loss_out = (float)(*lossp * inv_m_d);
    if (b && t < C) {
        const float g = ((dbp[t] + dbp[64 + t]) + dbp[128 + t]) + dbp[192 + t];
        float pb = b[t], m1 = mb[t], v1 = vb[t];
        adam_update(pb, m1, v1, g, coef);
        b[t] = pb;
        mb[t] = m1;
        vb[t] = v1;
    }
}

// Launch 2 of one model: K-block `blk`; every pointer is the model's own.
template <int NT>
__device__ __forceinline__ void small_update_body(
    const unsigned blk, const float *__restrict__ X, int64_t ldx, float *__restrict__ W,
    float *__restrict__ b, const int64_t *__restrict__ labels, int M, int K, int C, int n_blk,
    const float *__restrict__ P, const float *__restrict__ bias_copy, float inv_m, double inv_m_d,
    float *__restrict__ mW, float *__restrict__ vW, float *__restrict__ mb, float *__restrict__ vb,
    const AdamCoef &coef, float *__restrict__ loss_out, float *lds2) {
    constexpr int C16 = NT * 16, LDG = C16 + 1;
    float *gs = lds2 + kSmallScratch / 4;  // [M][LDG]
    float *xs = gs + M * LDG;              // [M][64]
    const int k0 = blk * kSmallBK;
    load_x_tile(X, ldx, M, K, k0, xs, kSmallBK);
    small_softmax_part<NT>(labels, M, C, n_blk, P, bias_copy, inv_m, gs);
    small_dw_part<NT>(k0, W, mW, vW, M, K, C, gs, xs, coef);
    if (blk != 0) return;  // (uniform per block)
    small_bias_part<NT>(b, mb, vb, M, C, gs, lds2, inv_m_d, coef, loss_out);
}

template <int NT>
__global__ __launch_bounds__(256) void adam_small_update_kernel(
    const float *__restrict__ X, int64_t ldx, float *__restrict__ W, float *__restrict__ b,
    const int64_t *__restrict__ labels, int M, int K, int C, int n_blk,
    const float *__restrict__ P, const float *__restrict__ bias_copy, float inv_m, double inv_m_d,
    float *__restrict__ mW, float *__restrict__ vW, float *__restrict__ mb, float *__restrict__ vb,
    AdamCoef coef, float *__restrict__ loss_out) {
    extern __shared__ __attribute__((aligned(16))) float lds2[];
    small_update_body<NT>(blockIdx.x, X, ldx, W, b, labels, M, K, C, n_blk, P, bias_copy, inv_m,
                          inv_m_d, mW, vW, mb, vb, coef, loss_out, lds2);
}

// Model i = blockIdx.y: its slices of W, b and the moments, its workspace area,
// its decay wd[i] (one uniform load: the "wd == 0" skip of adam_update stays a
// per-workgroup branch) and its loss slot loss_out[i * loss_stride].
template <int NT>
__global__ __launch_bounds__(256) void adam_sweep_update_kernel(
    const float *__restrict__ X, int64_t ldx, float *__restrict__ W, float *__restrict__ b,
    const int64_t *__restrict__ labels, int M, int K, int C, int n_blk,
    const float *__restrict__ ws, float inv_m, double inv_m_d, float *__restrict__ mW,
    float *__restrict__ vW, float *__restrict__ mb, float *__restrict__ vb, AdamCoef coef,
    const float *__restrict__ wd, float *__restrict__ loss_out, int64_t w_stride,
    int64_t ws_stride, int64_t loss_stride) {
    extern __shared__ __attribute__((aligned(16))) float sweep_lds2[];
    const int64_t i = blockIdx.y;
    coef.wd = wd[i];
    const float *area = ws + i * ws_stride;
    const int64_t ow = i * w_stride, ob = i * C;
    small_update_body<NT>(blockIdx.x, X, ldx, W + ow, b ? b + ob : nullptr, labels, M, K, C, n_blk,
                          area + kSweepBias, area, inv_m, inv_m_d, mW + ow, vW + ow,
                          b ? mb + ob : nullptr, b ? vb + ob : nullptr, coef,
                          loss_out ? loss_out + i * loss_stride : nullptr, sweep_lds2);
}

// The split form of the batched launch 2.  In the form above every K-block's
// workgroup re-sums all n_blk partial-logit blocks of its model and redoes the
// softmax: B n_blk^2 M C16 4 bytes of L2 reads per epoch.  Here one workgroup
// per model does that once (part 1), stores G [M][C16 + 1] to the model's
// workspace area (g_off floats into it) and finishes the bias and the loss
// (part 3); the K-block x model grid then loads G and its X tile and runs part
// 2.  Same parts, same sums in the same orders: the same bits.
template <int NT>
__global__ __launch_bounds__(256) void adam_sweep_softmax_kernel(
    float *__restrict__ b, const int64_t *__restrict__ labels, int M, int C, int n_blk,
    float *__restrict__ ws, float inv_m, double inv_m_d, float *__restrict__ mb,
    float *__restrict__ vb, AdamCoef coef, const float *__restrict__ wd,
    float *__restrict__ loss_out, int64_t ws_stride, int64_t g_off, int64_t loss_stride) {
    constexpr int LDG = NT * 16 + 1;
    extern __shared__ __attribute__((aligned(16))) float sweep_lds3[];
    float *gs = sweep_lds3 + kSmallScratch / 4;  // [M][LDG]
    const int64_t i = blockIdx.x;
    coef.wd = wd[i];
    float *area = ws + i * ws_stride;
    small_softmax_part<NT>(labels, M, C, n_blk, area + kSweepBias, area, inv_m, gs);
    float *G = area + g_off;
    for (int o = threadIdx.x; o < M * LDG; o += 256) G[o] = gs[o];
    const int64_t ob = i * C;
    small_bias_part<NT>(b ? b + ob : nullptr, b ? mb + ob : nullptr, b ? vb + ob : nullptr, M, C, gs,
                        sweep_lds3, inv_m_d, coef,
                        loss_out ? loss_out + i * loss_stride : nullptr);
}

template <int NT>
__global__ __launch_bounds__(256) void adam_sweep_dw_kernel(
    const float *__restrict__ X, int64_t ldx, float *__restrict__ W, int M, int K, int C,
    const float *__restrict__ ws, float *__restrict__ mW, float *__restrict__ vW, AdamCoef coef,
    const float *__restrict__ wd, int64_t w_stride, int64_t ws_stride, int64_t g_off) {
    constexpr int LDG = NT * 16 + 1;
    extern __shared__ __attribute__((aligned(16))) float sweep_lds4[];
    float *gs = sweep_lds4;    // [M][LDG]
    float *xs = gs + M * LDG;  // [M][64]
    const int64_t i = blockIdx.y;
    coef.wd = wd[i];
    const int k0 = blockIdx.x * kSmallBK;
    load_x_tile(X, ldx, M, K, k0, xs, kSmallBK);
    const float *G = ws + i * ws_stride + g_off;
    for (int o0 = threadIdx.x; o0 < M * LDG; o0 += 8 * 256) {  // (eight loads in flight)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = o0 + 256 * u < M * LDG ? G[o0 + 256 * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (o0 + 256 * u < M * LDG) gs[o0 + 256 * u] = v[u];
    }
    __syncthreads();
    const int64_t ow = i * w_stride;
    small_dw_part<NT>(k0, W + ow, mW + ow, vW + ow, M, K, C, gs, xs, coef);
}

bool small_eligible(int64_t M, int64_t K, int64_t C) {
    const int64_t C16 = (C + 15) / 16 * 16, n_blk = (K + kSmallBK - 1) / kSmallBK;
    return M >= 1 && M <= kSmallMaxM && C >= 1 && C <= 64 && K >= 1 && K < INT32_MAX - kSmallBK &&
           n_blk * M * C16 < INT32_MAX;
}

int64_t small_workspace(int64_t M, int64_t K, int64_t C) {
    if (!small_eligible(M, K, C)) return 0;
    const int64_t C16 = (C + 15) / 16 * 16, n_blk = (K + kSmallBK - 1) / kSmallBK;
    return 256 + al256(n_blk * M * C16 * 4) + 512;
}

// sgc_train_adam_f32's auto rule, from the A/B of scripts/adam_ab.py
// (profiles/adam/adam_ab.log).  Per epoch the small schedule
// measured about 2 + 0.29 M + 0.1 K / 64 us (19, 30, 43, 42 us at M = 60, 100,
// 120, 140) and the general one about 17 + 0.0195 K us (19, 22, 44, 90 us at
// K = 300, 500, 1433, 3703): small is the faster one where 16 M < K + 832.
// That holds at Pubmed, Cora and Citeseer (small measured 0.87, 0.96 and 0.48
// of general) and fails at the synthetic 100 x 300 x 5 (small 1.55 of general).
bool small_auto(int64_t M, int64_t K, int64_t C) {
    return small_eligible(M, K, C) && 16 * M < K + 832;
}

}  // namespace

int adam_set_tuning(int64_t value) {
    SGC_REQUIRE(value >= 0 && value <= 2, SGC_EINVAL,
                "adam_kernel must be 0 (auto), 1 (general) or 2 (small)");
    g_adam_kernel = (int)value;
    return SGC_OK;
}

int adam_sweep_set_form(int64_t value) {
    SGC_REQUIRE(value >= 0 && value <= 2, SGC_EINVAL,
                "adam_sweep_form must be 0 (auto), 1 (fused) or 2 (split)");
    g_adam_sweep_form = (int)value;
    return SGC_OK;
}

int64_t adam_small_max_rows() { return kSmallMaxM; }

int adam_step(int32_t n_tensors, float *const *params, const float *const *grads,
              float *const *exp_avgs, float *const *exp_avg_sqs, const int64_t *numels,
              int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
              hipStream_t s) {
    SGC_REQUIRE(n_tensors >= 1 && n_tensors <= kMaxTensors, SGC_EINVAL,
                "adam_step: n_tensors=%d outside 1..%d", n_tensors, kMaxTensors);
    SGC_REQUIRE(step >= 1, SGC_EINVAL, "adam_step: step=%lld < 1", (long long)step);
    SGC_REQUIRE(params && grads && exp_avgs && exp_avg_sqs && numels, SGC_EINVAL,
                "adam_step: null pointer table");
    AdamTensors T;
    int64_t blocks = 0;
    for (int i = 0; i < kMaxTensors; ++i) {
        T.p[i] = T.m[i] = T.v[i] = nullptr;
        T.g[i] = nullptr;
        T.n[i] = 0;
        T.blk0[i] = (int32_t)blocks;
        if (i >= n_tensors) continue;
        SGC_REQUIRE(numels[i] >= 0, SGC_EINVAL, "adam_step: numels[%d]=%lld < 0", i,
                    (long long)numels[i]);
        if (!grads[i] || numels[i] == 0) continue;  // skipped: nothing of it moves
        SGC_REQUIRE(params[i] && exp_avgs[i] && exp_avg_sqs[i], SGC_EINVAL,
                    "adam_step: null parameter or moment %d", i);
        T.p[i] = params[i];
        T.g[i] = grads[i];
        T.m[i] = exp_avgs[i];
        T.v[i] = exp_avg_sqs[i];
        T.n[i] = numels[i];
        blocks += (numels[i] + kStepPerBlock - 1) / kStepPerBlock;
        SGC_REQUIRE(blocks < INT32_MAX, SGC_ERANGE, "adam_step: too many elements");
    }
    T.blk0[kMaxTensors] = (int32_t)blocks;
    if (blocks == 0) return SGC_OK;
    const AdamCoef coef = adam_coef(step, lr, beta1, beta2, eps, weight_decay);
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T, coef);
    const hipError_t e = hipGetLastError();
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "adam_step launch failed: %s", hipGetErrorString(e));
    return SGC_OK;
}


int64_t train_adam_workspace(int64_t M, int64_t K, int64_t C) {
    if (M <= 0 || K <= 0 || C <= 0 || C > 64) return 0;
    return std::max(xent_workspace_bytes(M, K, C), small_workspace(M, K, C));
}

int train_adam(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels, int64_t M,
               int64_t K, int64_t C, float *mW, float *vW, float *mb, float *vb, int64_t step0,
               int32_t epochs, double lr, double beta1, double beta2, double eps,
               double weight_decay, float *loss_trace, void *ws, int64_t ws_bytes,
               hipStream_t s) {
    SGC_REQUIRE(epochs >= 0, SGC_EINVAL, "train_adam: epochs=%d < 0", epochs);
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && C <= 64 && ldx >= K, SGC_EINVAL,
                "train_adam: bad shape M=%lld K=%lld C=%lld ldx=%lld (1 <= C <= 64, ldx >= K)",
                (long long)M, (long long)K, (long long)C, (long long)ldx);
    SGC_REQUIRE(step0 >= 0, SGC_EINVAL, "train_adam: step0=%lld < 0", (long long)step0);
    SGC_REQUIRE(b ? (mb && vb) : (!mb && !vb), SGC_EINVAL,
                "train_adam: b and its two moments must be given or NULL together");
    SGC_REQUIRE(X && W && labels && mW && vW && ws, SGC_EINVAL, "train_adam: null pointer");
    if (const int rc = xent_adam_check(M, K, C, ldx)) return rc;
    const int64_t need = train_adam_workspace(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "train_adam: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    if (epochs == 0) return SGC_OK;
    const bool small = small_eligible(M, K, C) &&
                       (g_adam_kernel == 2 || (g_adam_kernel == 0 && small_auto(M, K, C)));
    g_adam_kernel_last = small ? 2 : 1;
    if (!small) {
        for (int e = 0; e < epochs; ++e) {
            const AdamCoef coef = adam_coef(step0 + e + 1, lr, beta1, beta2, eps, weight_decay);
            if (const int rc = xent_adam_epoch(X, ldx, W, b, labels, M, K, C, mW, vW, mb, vb, coef,
                                               loss_trace ? loss_trace + e : nullptr, ws, ws_bytes,
                                               s))
                return rc;
        }
        return SGC_OK;
    }
    const int NT = (int)((C + 15) / 16), C16 = NT * 16;
    const int n_blk = (int)((K + kSmallBK - 1) / kSmallBK);
    char *p = (char *)(((uintptr_t)ws + 255) & ~uintptr_t(255));
    float *bias_copy = (float *)p;
    float *P = (float *)(p + 256);
    const size_t lds1 = (size_t)small_lds1(M, C16), lds2 = (size_t)small_lds2(M, C16);
    const void *k2 = NT == 1   ? (const void *)adam_small_update_kernel<1>
                     : NT == 2 ? (const void *)adam_small_update_kernel<2>
                     : NT == 3 ? (const void *)adam_small_update_kernel<3>
                               : (const void *)adam_small_update_kernel<4>;
    int cus = 0;
    SGC_HIP_CHECK(persistent_setup((const void *)adam_small_logits_kernel, &cus));
    SGC_HIP_CHECK(persistent_setup(k2, &cus));
    const float inv_m = 1.0f / (float)M;
    const double inv_m_d = 1.0 / (double)M;
    for (int e = 0; e < epochs; ++e) {
        const AdamCoef coef = adam_coef(step0 + e + 1, lr, beta1, beta2, eps, weight_decay);
        float *loss_out = loss_trace ? loss_trace + e : nullptr;
        hipLaunchKernelGGL(adam_small_logits_kernel, dim3(n_blk), dim3(256), lds1, s, X, ldx, W, b,
                           (int)M, (int)K, (int)C, C16, P, bias_copy);
#define SGC_ADAM_SMALL(N)                                                                        \
    hipLaunchKernelGGL(adam_small_update_kernel<N>, dim3(n_blk), dim3(256), lds2, s, X, ldx, W, \
                       b, labels, (int)M, (int)K, (int)C, n_blk, P, bias_copy, inv_m, inv_m_d,  \
                       mW, vW, mb, vb, coef, loss_out)
        switch (NT) {
            case 1: SGC_ADAM_SMALL(1); break;
            case 2: SGC_ADAM_SMALL(2); break;
            case 3: SGC_ADAM_SMALL(3); break;
            default: SGC_ADAM_SMALL(4); break;
        }
#undef SGC_ADAM_SMALL
        const hipError_t err = hipGetLastError();
        SGC_REQUIRE(err == hipSuccess, SGC_EHIP, "train_adam launch failed: %s",
                    hipGetErrorString(err));
    }
    return SGC_OK;
}

// ---- the weight-decay sweep: B models on one X --------------------------------
// Workspace of the batched small schedule: after the 256-B alignment slack,
// one area per model -- its bias copy (256 B), its partial logits, then G
// [M][C16 + 1] (written by the split form only).
static int64_t sweep_area_bytes(int64_t M, int64_t K, int64_t C) {
    const int64_t C16 = (C + 15) / 16 * 16, n_blk = (K + kSmallBK - 1) / kSmallBK;
    return kSweepBias * 4 + al256(n_blk * M * C16 * 4) + al256(M * (C16 + 1) * 4);
}
// (floats from an area's start to its G: the split form's softmax - onehot)
static int64_t sweep_g_offset(int64_t M, int64_t K, int64_t C) {
    const int64_t C16 = (C + 15) / 16 * 16, n_blk = (K + kSmallBK - 1) / kSmallBK;
    return (kSweepBias * 4 + al256(n_blk * M * C16 * 4)) / 4;
}

// The form of the batched launch 2 (see adam_sweep_softmax_kernel), from the
// A/B of scripts/adam_sweep_ab.py (profiles/adam_sweep/ab.log).
// The split form pays one more launch per epoch (2 - 3 us: slower at every
// B = 1 and at 8 models of Pubmed's and Cora's shape) and saves the fused
// form's redundant reads, B n_blk^2 M C16 4 bytes per epoch.  The largest
// measured loss was at 38 MB of them (Cora, B = 8: 47.8 -> 49.3 us per epoch),
// the smallest measured gain at 206 MB (Citeseer, B = 8: 60.4 -> 52.1 us;
// 1.55 GB at Citeseer B = 60: 307 -> 158 us): split from 100 MB up.
static bool sweep_split(int64_t B, int64_t M, int64_t K, int64_t C) {
    if (g_adam_sweep_form) return g_adam_sweep_form == 2;
    const int64_t C16 = (C + 15) / 16 * 16, n_blk = (K + kSmallBK - 1) / kSmallBK;
    return B * n_blk * n_blk * M * C16 * 4 >= 100 * 1000 * 1000;
}

int64_t train_adam_sweep_workspace(int64_t B, int64_t M, int64_t K, int64_t C) {
    if (B < 1 || B > kSweepMaxModels || M <= 0 || K <= 0 || C <= 0 || C > 64) return 0;
    const int64_t batched = small_eligible(M, K, C) ? 256 + B * sweep_area_bytes(M, K, C) : 0;
    return std::max(xent_workspace_bytes(M, K, C), batched);
}

// The batched small schedule wherever small_eligible holds and "adam_kernel" is
// not 1: small_auto's crossover was measured for one model, whose two launches
// leave most of the machine idle; nobody has measured where a batch crosses
// over, so the sweep does not apply it.  Everything else -- M > kSmallMaxM,
// "adam_kernel" = 1 -- runs the general schedule model by model.
int train_adam_sweep(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                     int64_t B, int64_t M, int64_t K, int64_t C, float *mW, float *vW, float *mb,
                     float *vb, int64_t step0, int32_t epochs, double lr, double beta1,
                     double beta2, double eps, const float *wd_dev, float *loss_trace, void *ws,
                     int64_t ws_bytes, hipStream_t s) {
    SGC_REQUIRE(epochs >= 0, SGC_EINVAL, "train_adam_sweep: epochs=%d < 0", epochs);
    SGC_REQUIRE(B >= 1 && B <= kSweepMaxModels, SGC_EINVAL, "train_adam_sweep: B=%lld outside 1..%d",
                (long long)B, kSweepMaxModels);
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && C <= 64 && ldx >= K, SGC_EINVAL,
                "train_adam_sweep: bad shape M=%lld K=%lld C=%lld ldx=%lld (1 <= C <= 64, ldx >= K)",
                (long long)M, (long long)K, (long long)C, (long long)ldx);
    SGC_REQUIRE(step0 >= 0, SGC_EINVAL, "train_adam_sweep: step0=%lld < 0", (long long)step0);
    SGC_REQUIRE(b ? (mb && vb) : (!mb && !vb), SGC_EINVAL,
                "train_adam_sweep: b and its two moments must be given or NULL together");
    SGC_REQUIRE(wd_dev, SGC_EINVAL, "train_adam_sweep: null weight_decay_dev");
    SGC_REQUIRE(X && W && labels && mW && vW && ws, SGC_EINVAL, "train_adam_sweep: null pointer");
    if (const int rc = xent_adam_check(M, K, C, ldx)) return rc;
    const int64_t need = train_adam_sweep_workspace(B, M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "train_adam_sweep: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    if (epochs == 0) return SGC_OK;
    const bool batched = small_eligible(M, K, C) && g_adam_kernel != 1;
    g_adam_sweep_last = batched ? 2 : 1;
    const int64_t w_stride = C * K;
    if (!batched) {
        for (int64_t i = 0; i < B; ++i) {
            const int64_t ow = i * w_stride, ob = i * C;
            for (int e = 0; e < epochs; ++e) {
                // (coef.wd is a placeholder: the last launch reads wd_dev[i])
                const AdamCoef coef = adam_coef(step0 + e + 1, lr, beta1, beta2, eps, 0.0);
                if (const int rc = xent_adam_epoch(
                        X, ldx, W + ow, b ? b + ob : nullptr, labels, M, K, C, mW + ow, vW + ow,
                        b ? mb + ob : nullptr, b ? vb + ob : nullptr, coef,
                        loss_trace ? loss_trace + i * epochs + e : nullptr, ws, ws_bytes, s,
                        wd_dev + i))
                    return rc;
            }
        }
        return SGC_OK;
    }
    const int NT = (int)((C + 15) / 16), C16 = NT * 16;
    const int n_blk = (int)((K + kSmallBK - 1) / kSmallBK);
    float *area0 = (float *)(((uintptr_t)ws + 255) & ~uintptr_t(255));
    const int64_t ws_stride = sweep_area_bytes(M, K, C) / 4;
    const size_t lds1 = (size_t)small_lds1(M, C16), lds2 = (size_t)small_lds2(M, C16);
    const bool split = sweep_split(B, M, K, C);
    g_adam_sweep_form_last = split ? 2 : 1;
    int cus = 0;
    SGC_HIP_CHECK(persistent_setup((const void *)adam_sweep_logits_kernel, &cus));
#define SGC_ADAM_SWEEP_SETUP(N)                                                              \
    do {                                                                                     \
        SGC_HIP_CHECK(persistent_setup((const void *)adam_sweep_update_kernel<N>, &cus));    \
        SGC_HIP_CHECK(persistent_setup((const void *)adam_sweep_softmax_kernel<N>, &cus));   \
        SGC_HIP_CHECK(persistent_setup((const void *)adam_sweep_dw_kernel<N>, &cus));        \
    } while (0)
    switch (NT) {
        case 1: SGC_ADAM_SWEEP_SETUP(1); break;
        case 2: SGC_ADAM_SWEEP_SETUP(2); break;
        case 3: SGC_ADAM_SWEEP_SETUP(3); break;
        default: SGC_ADAM_SWEEP_SETUP(4); break;
    }
#undef SGC_ADAM_SWEEP_SETUP
    const int64_t g_off = sweep_g_offset(M, K, C);
    const size_t lds3 = (size_t)(kSmallScratch + M * (C16 + 1) * 4);
    const size_t lds4 = (size_t)((M * (C16 + 1) + M * kSmallBK) * 4);
    const float inv_m = 1.0f / (float)M;
    const double inv_m_d = 1.0 / (double)M;
    const dim3 grid((unsigned)n_blk, (unsigned)B);
    for (int e = 0; e < epochs; ++e) {
        const AdamCoef coef = adam_coef(step0 + e + 1, lr, beta1, beta2, eps, 0.0);
        float *loss_out = loss_trace ? loss_trace + e : nullptr;
        hipLaunchKernelGGL(adam_sweep_logits_kernel, grid, dim3(256), lds1, s, X, ldx, W, b, (int)M,
                           (int)K, (int)C, C16, area0, w_stride, ws_stride);
#define SGC_ADAM_SWEEP(N)                                                                          \
    if (split) {                                                                                  \
        hipLaunchKernelGGL(adam_sweep_softmax_kernel<N>, dim3((unsigned)B), dim3(256), lds3, s, b, \
                           labels, (int)M, (int)C, n_blk, area0, inv_m, inv_m_d, mb, vb, coef,    \
                           wd_dev, loss_out, ws_stride, g_off, (int64_t)epochs);                  \
        hipLaunchKernelGGL(adam_sweep_dw_kernel<N>, grid, dim3(256), lds4, s, X, ldx, W, (int)M,  \
                           (int)K, (int)C, area0, mW, vW, coef, wd_dev, w_stride, ws_stride,      \
                           g_off);                                                                \
    } else                                                                                        \
        hipLaunchKernelGGL(adam_sweep_update_kernel<N>, grid, dim3(256), lds2, s, X, ldx, W, b,   \
                           labels, (int)M, (int)K, (int)C, n_blk, area0, inv_m, inv_m_d, mW, vW,  \
                           mb, vb, coef, wd_dev, loss_out, w_stride, ws_stride, (int64_t)epochs)
        switch (NT) {
            case 1: SGC_ADAM_SWEEP(1); break;
            case 2: SGC_ADAM_SWEEP(2); break;
            case 3: SGC_ADAM_SWEEP(3); break;
            default: SGC_ADAM_SWEEP(4); break;
        }
#undef SGC_ADAM_SWEEP
        const hipError_t err = hipGetLastError();
        SGC_REQUIRE(err == hipSuccess, SGC_EHIP, "train_adam_sweep launch failed: %s",
                    hipGetErrorString(err));
    }
    return SGC_OK;
}

// One host call, the existing launch chain once per model on the one
// workspace: the stream orders model i + 1's chain behind model i's.
int linear_eval_sweep_f32(const float *X, int64_t ldx, const float *W, const float *b,
                          const int64_t *labels, int64_t B, int64_t M, int64_t K, int64_t C,
                          int64_t *pred, int64_t *confusion, int64_t *counts, float *loss, void *ws,
                          int64_t ws_bytes, hipStream_t s) {
    SGC_REQUIRE(B >= 1 && B <= kSweepMaxModels, SGC_EINVAL,
                "linear_eval_sweep: B=%lld outside 1..%d", (long long)B, kSweepMaxModels);
    for (int64_t i = 0; i < B; ++i)
        // (a bad argument fails model 0's call, before any launch)
        if (const int rc = linear_eval_f32(
                X, ldx, W ? W + i * C * K : nullptr, b ? b + i * C : nullptr, labels, M, K, C,
                pred ? pred + i * M : nullptr, confusion ? confusion + i * C * C : nullptr,
                counts ? counts + 2 * i : nullptr, loss ? loss + i : nullptr, ws, ws_bytes, s))
            return rc;
    return SGC_OK;
}

SGC_WARM_UNIT(warm_adam)

}  // namespace sgc
