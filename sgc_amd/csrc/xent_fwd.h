// xent_fwd.h -- launch A of the fused classifier step (xent.hip): logits on
// the LDS block tile, row softmax / log-sum-exp, G and the per-wave loss and dG
// partials.  Two units instantiate it: xent.hip with NoStop alone and
// xent_fwd_stop.hip with StopWord alone (stop_policy.h) -- a second set of this
// kernel in xent.hip's unit changed the register allocation of the first.
// Everything here has internal linkage: each including unit owns its
// instantiations.
#pragma once
#include "gemm_tile.h"
#include "group16.h"
#include "stop_policy.h"

namespace sgc {

namespace {

// ---- A: logits -> G, loss / dG partials ------------------------------------
template <int V, int NT, int NB, class Stop>
__global__ __launch_bounds__(256) void xent_fwd_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W,
    const float *__restrict__ b, const int64_t *__restrict__ labels, int M, int K, int C,
    float inv_m, float *__restrict__ G, int ldg, double *__restrict__ loss_part,
    float *__restrict__ db_part, float *__restrict__ logits, int64_t ldl, Stop stop) {
    __shared__ LdsTile<V, NT, NB> sm;
    if (stop.set()) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wave = blockIdx.x * 4 + w;
    const int i = lane & 15, g = lane >> 4;
    const int m_blk = blockIdx.x * kLdsBM;
    const int m0 = m_blk + w * 32;
    double wave_loss = 0.0;
    float dbc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dbc[n] = 0.f;
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
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    z[n] = valid[n] ? acc[t][n][r] + bias[n] : -INFINITY;
                    mx = fmaxf(mx, z[n]);
                }
                mx = group16_max(mx);
                float se = 0.f;
                float ez[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    ez[n] = valid[n] ? expf(z[n] - mx) : 0.f;
                    se += ez[n];
                }
                se = group16_sum(se);
                // p = exp(z - max) / sum and loss = (max - z_y) + log(sum): as
                // softmax itself, independent of a common offset of the row
                // (lse = max + log(sum), rounded to ulp(|lse|), put |lse| * 6e-8
                // into exp(z - lse) and lse - z_y; loss.hip's note)
                const float ls = logf(se);
                const int64_t y = row_ok ? labels[m] : -1;
                float zy = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int c = n * 16 + i;
                    const bool is_y = (c == y);
                    if (is_y) zy = z[n];
                    const float p = ez[n] / se;
                    const float gv = row_ok ? (p - (is_y ? 1.f : 0.f)) * inv_m : 0.f;
                    if (row_ok) {
                        G[(int64_t)m * ldg + c] = gv;
                        if (logits && valid[n]) logits[(int64_t)m * ldl + c] = z[n];
                    }
                    dbc[n] += gv;
                }
                zy = group16_sum(zy);  // exactly one lane of the group holds z_y
                if (row_ok && i == 0) wave_loss += (double)((mx - zy) + ls);
            }
    }
    // per-wave partials: loss (lanes i==0 of each group), dG column sums
    double l = wave_loss;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (lane == 0) loss_part[wave] = l;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        float s = dbc[n];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g == 0) db_part[(int64_t)wave * ldg + n * 16 + i] = s;
    }
}

// Launch A over ceil(M / 128) blocks with one policy: the (V, NT, NB) table of
// gemm_tile.h's dispatch_tile.
template <class Stop>
hipError_t launch_xent_fwd(Stop stop, int V, int NT, int NB, const float *X, int64_t ldx,
                           const float *W, const float *b, const int64_t *labels, int M, int K,
                           int C, float *G, int ldg, double *loss_part, float *db_part,
                           float *logits, int64_t ldl, hipStream_t s) {
    const int blocks = (M + kLdsBM - 1) / kLdsBM;
    const float inv_m = 1.0f / (float)M;
    dispatch_tile(V, NT, NB, [&](auto v, auto nt, auto nb) {
        hipLaunchKernelGGL(
            (xent_fwd_kernel<decltype(v)::value, decltype(nt)::value, decltype(nb)::value, Stop>),
            dim3(blocks), dim3(256), 0, s, X, ldx, W, b, labels, M, K, C, inv_m, G, ldg, loss_part,
            db_part, logits, ldl, stop);
    });
    return hipGetLastError();
}

}  // namespace
}  // namespace sgc
