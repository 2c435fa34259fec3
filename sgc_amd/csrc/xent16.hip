// xent16.hip -- the fused SGC classifier training step on 16-bit features
// (torch.bfloat16 / torch.float16 X; W, b, G, loss, dW and db fp32): xent.hip's
// launch structure with X read twice at 16 bits, and the two training loops
// built on it (sgc_train_adam_x16, sgc_train_lbfgs_x16's closure).
//
//   A  xent_fwd_x16_kernel   logits by the split-bf16 scheme on linear_x16_kernel's
//                            stream (linear16.hip: persistent workgroups, W's
//                            image built behind the first loads, the slot ring,
//                            every load issued on every path); each finished
//                            16-row tile is followed at once by xent_fwd_kernel's
//                            row epilogue (same formulas): G -> global [M][C16]
//                            (fp32, padded classes 0) and the tile's loss partial;
//   B  xent_dw_cols_x16_kernel (linear16.hip) dW partials over column blocks x
//                            row ranges, db partials from the same G loads
//                            (its db_slab path, in the stepwise and the fused
//                            loops alike);
//   C  xent16_reduce_kernel  partials -> dW, db and the loss in one launch, each
//                            in a fixed order; with ADAM the finished gradient
//                            element is applied to W / b in place (adam_update.h).
//
// The loss partial is per 16-row TILE, indexed by tile number: the waves of
// launch A take tiles dynamically, so which wave computes which tile differs
// run to run and a per-wave partial would not be reproducible.  Each tile's
// partial is a fixed tree over its 16 rows, and C sums the tiles in a fixed
// order: loss, dW and db are bitwise reproducible run to run.
//
// Stop-aware forms (sgc_train_lbfgs_x16): A and C take the L-BFGS state's stop
// word as a nullable first argument, test it with one wave-uniform load at entry
// and return when it is set; B exists a second time as
// xent_dw_cols_x16_stop_kernel, a second wrapper of x16::dw_cols compiled in
// this unit.
#include <algorithm>
#include <cstring>

#include "adam_update.h"
#include "x16_stream.h"

namespace sgc {

namespace {

// ---- A: logits -> G, per-tile loss partials ---------------------------------
// x16::stream (x16_stream.h) behind the stop test; what is here is the end of
// a tile.  Lane (j, kg) then holds row j of the tile and classes 16 n + 4 kg + r
// (n < NT, r < 4), so a row's reductions run over r and n in the lane, then
// across the four lanes j, j + 16, j + 32, j + 48 (xor 16, xor 32: every lane
// of the four ends with the same bits).  Nothing is held: G and the tile's
// partial go out as the tile finishes, through descriptors of the tile's own
// rows (rows past M lie outside them and are dropped), so no offset depends
// on M.  The tile's labels are read at wave-uniform addresses (rows past M
// clamped to the last row, their loss masked).
template <int NT, int NW, typename XT>
__global__ __launch_bounds__(64 * NW) void xent_fwd_x16_kernel(
    const int64_t *__restrict__ stop, const XT *__restrict__ X, int64_t ldx,
    const float *__restrict__ W, const float *__restrict__ b, const int64_t *__restrict__ labels,
    int M, int K, int C, float inv_m, float *__restrict__ G, int ldg,
    double *__restrict__ loss_tile) {
    using namespace x16;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) u32x4 sgx16[];
    if (stop && *stop != 0) return;  // (uniform for the grid: no barrier reached)
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, kg = lane >> 4;
    // the loss partials: one double per tile (n_tiles * 8 < 2^31)
    const auto ld = __builtin_amdgcn_make_buffer_rsrc(loss_tile, 0, ((M + 15) >> 4) * 8, 0x00020000);
    const uint32_t glane = (uint32_t)(j * ldg + 4 * kg) * 4u;  // row j, class 4 kg of its tile
    stream<NT, NW, XT>(reinterpret_cast<char *>(sgx16), X, ldx, W, b, M, K, C,
                       [&](int tile, f4 (&z)[NT]) {
        const int row0 = tile * 16;
        const int rows = min(16, M - row0);  // uniform, >= 1
        const bool row_ok = j < rows;
        // the tile's labels, uniform addresses; lane (j, .) keeps row j's
        int y = -1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t yi = labels[row0 + min(i, rows - 1)];
            const int ys = (yi >= 0 && yi < C) ? (int)yi : -1;
            y = (j == i) ? ys : y;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (n * 16 + 4 * kg + r >= C) z[n][r] = -INFINITY;
                mx = fmaxf(mx, z[n][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        f4 ez[NT];
        float se = 0.f;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ez[n][r] = n * 16 + 4 * kg + r < C ? expf(z[n][r] - mx) : 0.f;
                se += ez[n][r];
            }
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        // p = exp(z - max) / sum and loss = (max - z_y) + log(sum), as xent_fwd_kernel
        const float ls = logf(se);
        float zy = 0.f;
        const auto gd = __builtin_amdgcn_make_buffer_rsrc(G + (int64_t)row0 * ldg, 0,
                                                          rows * ldg * 4, 0x00020000);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            f4 gv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cl = n * 16 + 4 * kg + r;
                const bool is_y = cl == y;
                if (is_y) zy = z[n][r];
                const float p = ez[n][r] / se;
                gv[r] = cl < C ? (p - (is_y ? 1.f : 0.f)) * inv_m : 0.f;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, gv), gd,
                                                   glane + 64u * n, 0, 0);
        }
        zy += __shfl_xor(zy, 16, 64);  // exactly one lane of the four holds z_y
        zy += __shfl_xor(zy, 32, 64);
        double l = row_ok ? (double)((mx - zy) + ls) : 0.0;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) l += __shfl_xor(l, o, 64);  // the 16 rows, a fixed tree
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, l), ld,
                                              lane == 0 ? (uint32_t)tile * 8u : kOffOOB, 0, 0);
    });
}

// ---- B behind the stop word: the second form of xent_dw_cols_x16_kernel -------
template <int NT, typename XT>
__global__ __launch_bounds__(256) void xent_dw_cols_x16_stop_kernel(
    const int64_t *__restrict__ stop, const XT *__restrict__ X, int64_t ldx,
    const float *__restrict__ G, int ldg, int M, int K, int C, int n_cblk, int R,
    float *__restrict__ slab, float *__restrict__ db_slab) {
    if (*stop != 0) return;
    x16::dw_cols<NT, XT>(X, ldx, G, ldg, M, K, C, n_cblk, R, slab, db_slab);
}

// ---- C: the fixed-order reductions, one launch --------------------------------
// Blocks [0, dw_blocks): 64 dW elements each, xent_reduce_dw_db_kernel's order
//   (wave w a quarter of the partials in order, batches of 16 loads, then the
//   four quarters in order);
// blocks dw_blocks + i (i < db_blocks): db, a wave per class (lane l sums
//   partials l, l + 64, ..., then a fixed xor tree);
// the last block: the loss -- thread t sums tiles t, t + 256, ... in order, then
//   a fixed-shape LDS tree, in double.
// ADAM: the thread that holds a finished gradient element applies it to W / b
// and the moments in place (db blocks skipped when b is null; the loss block
// when loss is null); else the elements go to dW / db (db blocks skipped when
// db is null) and *loss.
template <bool ADAM>
__global__ __launch_bounds__(256) void xent16_reduce_kernel(
    const int64_t *__restrict__ stop, const float *__restrict__ slab, int n_parts, int C, int K,
    int C16, int dw_blocks, int db_blocks, const float *__restrict__ db_slab,
    const double *__restrict__ loss_tile, int n_tiles, double inv_m, float *__restrict__ dW,
    float *__restrict__ db, float *__restrict__ loss, float *__restrict__ mW,
    float *__restrict__ vW, float *__restrict__ mb, float *__restrict__ vb, AdamCoef coef) {
    __shared__ float part[4][64];
    __shared__ double red[256];
    if (stop && *stop != 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int blk = (int)blockIdx.x;
    if (blk < dw_blocks) {
        const int j0 = (int)((int64_t)n_parts * w / 4), j1 = (int)((int64_t)n_parts * (w + 1) / 4);
        const int64_t e = blk * 64LL + lane;
        const bool ok = e < (int64_t)C * K;
        float s = 0.f;
        if (ok) {
            const int64_t cls = e / K, k = e - cls * K;
            const float *p = slab + cls * K + k;
            const int64_t stride = (int64_t)C16 * K;
            for (int j = j0; j < j1; j += 16) {
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = j + u < j1 ? p[(int64_t)(j + u) * stride] : 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u) s += v[u];
            }
        }
        part[w][lane] = s;
        __syncthreads();
        if (w == 0 && ok) {
            const float g = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
            if constexpr (ADAM) {
                float pw = dW[e], m = mW[e], v = vW[e];  // (dW is W here)
                adam_update(pw, m, v, g, coef);
                dW[e] = pw;
                mW[e] = m;
                vW[e] = v;
            } else {
                dW[e] = g;
            }
        }
        return;  // (uniform per block)
    }
    if (blk < dw_blocks + db_blocks) {
        const int cls = (blk - dw_blocks) * 4 + w;
        if (cls < C) {
            const float *p = db_slab + cls;
            float s = 0.f;
            for (int jj = lane; jj < n_parts; jj += 64) s += p[(int64_t)jj * C16];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) {
                if constexpr (ADAM) {
                    float pb = db[cls], m = mb[cls], v = vb[cls];  // (db is b here)
                    adam_update(pb, m, v, s, coef);
                    db[cls] = pb;
                    mb[cls] = m;
                    vb[cls] = v;
                } else {
                    db[cls] = s;
                }
            }
        }
        return;
    }
    const int t = threadIdx.x;
    double s = 0.0;
    for (int jj = t; jj < n_tiles; jj += 256) s += loss_tile[jj];
    red[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) *loss = (float)(red[0] * inv_m);
}

template <int NT, typename XT>
hipError_t launch_fwd(const int64_t *stop, const void *X, int64_t ldx, const float *W,
                      const float *b, const int64_t *labels, int M, int K, int C, float *G, int ldg,
                      double *loss_tile, hipStream_t s) {
    int blocks = 0;
    const hipError_t e = x16::persistent_grid(
        reinterpret_cast<const void *>(&xent_fwd_x16_kernel<NT, x16::kWaves, XT>), M, &blocks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((xent_fwd_x16_kernel<NT, x16::kWaves, XT>), dim3((unsigned)blocks),
                       dim3(64 * x16::kWaves), x16::image_lds(K, C), s, stop,
                       static_cast<const XT *>(X), ldx, W, b, labels, M, K, C, 1.0f / (float)M, G,
                       ldg, loss_tile);
    return hipGetLastError();
}

template <typename XT>
hipError_t dispatch_fwd(int nt, const int64_t *stop, const void *X, int64_t ldx, const float *W,
                        const float *b, const int64_t *labels, int M, int K, int C, float *G,
                        int ldg, double *loss_tile, hipStream_t s) {
    switch (nt) {
        case 1: return launch_fwd<1, XT>(stop, X, ldx, W, b, labels, M, K, C, G, ldg, loss_tile, s);
        case 2: return launch_fwd<2, XT>(stop, X, ldx, W, b, labels, M, K, C, G, ldg, loss_tile, s);
        default: return launch_fwd<3, XT>(stop, X, ldx, W, b, labels, M, K, C, G, ldg, loss_tile, s);
    }
}

// launch B behind the stop word: linear16.hip's grid, the second form of its kernel
template <int NT, typename XT>
hipError_t launch_dw_stop(const int64_t *stop, const void *X, int64_t ldx, const float *G, int ldg,
                          int M, int K, int C, int R, float *slab, float *db_slab, hipStream_t s) {
    int n_cblk = 0;
    const int blocks = x16::dw_cols_blocks(K, R, &n_cblk);
    hipLaunchKernelGGL((xent_dw_cols_x16_stop_kernel<NT, XT>), dim3(blocks), dim3(256), 0, s, stop,
                       static_cast<const XT *>(X), ldx, G, ldg, M, K, C, n_cblk, R, slab, db_slab);
    return hipGetLastError();
}

template <typename XT>
hipError_t dispatch_dw_stop(int nt, const int64_t *stop, const void *X, int64_t ldx, const float *G,
                            int ldg, int M, int K, int C, int R, float *slab, float *db_slab,
                            hipStream_t s) {
    switch (nt) {
        case 1: return launch_dw_stop<1, XT>(stop, X, ldx, G, ldg, M, K, C, R, slab, db_slab, s);
        case 2: return launch_dw_stop<2, XT>(stop, X, ldx, G, ldg, M, K, C, R, slab, db_slab, s);
        default: return launch_dw_stop<3, XT>(stop, X, ldx, G, ldg, M, K, C, R, slab, db_slab, s);
    }
}

// Where the launches keep G and their partials in the workspace.
struct Parts {
    float *G, *slab, *db_slab;
    double *loss_tile;
    int C16, R, n_tiles;
};

Parts carve(void *ws, int64_t M, int64_t K, int64_t C) {
    Parts o;
    o.C16 = (int)((C + 15) / 16 * 16);
    o.R = dw_cols_x16_ranges(M);
    o.n_tiles = (int)((M + 15) / 16);
    char *p = (char *)(((uintptr_t)ws + 255) & ~uintptr_t(255));
    o.G = (float *)p;
    p += al256(M * o.C16 * 4);
    o.loss_tile = (double *)p;
    p += al256((int64_t)o.n_tiles * 8);
    o.slab = (float *)p;
    p += al256((int64_t)o.R * o.C16 * K * 4);
    o.db_slab = (float *)p;
    return o;
}

// Launches A and B (arguments and workspace checked by the caller).
int launch_ab(const int64_t *stop, const void *X, int32_t x_dtype, int64_t ldx, const float *W,
              const float *b, const int64_t *labels, int64_t M, int64_t K, int64_t C,
              const Parts &o, hipStream_t s) {
    const int nt = o.C16 / 16;
    const bool bf = x_dtype == SGC_DTYPE_BF16;
    hipError_t e = bf ? dispatch_fwd<bf16_t>(nt, stop, X, ldx, W, b, labels, (int)M, (int)K, (int)C,
                                             o.G, o.C16, o.loss_tile, s)
                      : dispatch_fwd<f16_t>(nt, stop, X, ldx, W, b, labels, (int)M, (int)K, (int)C,
                                            o.G, o.C16, o.loss_tile, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_xent_x16 launch A failed: %s",
                hipGetErrorString(e));
    if (!stop)
        e = launch_dw_cols_x16(X, x_dtype, ldx, o.G, o.C16, (int)M, (int)K, (int)C, o.slab,
                               o.db_slab, s);
    else
        e = bf ? dispatch_dw_stop<bf16_t>(nt, stop, X, ldx, o.G, o.C16, (int)M, (int)K, (int)C, o.R,
                                          o.slab, o.db_slab, s)
               : dispatch_dw_stop<f16_t>(nt, stop, X, ldx, o.G, o.C16, (int)M, (int)K, (int)C, o.R,
                                         o.slab, o.db_slab, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "linear_xent_x16 launch B failed: %s",
                hipGetErrorString(e));
    return SGC_OK;
}

// The three launches of the step; stop: null, or the word behind which all three run.
int step_launches(const int64_t *stop, const void *X, int32_t x_dtype, int64_t ldx, const float *W,
                  const float *b, const int64_t *labels, int64_t M, int64_t K, int64_t C,
                  float *loss, float *dW, float *db, void *ws, hipStream_t s) {
    const Parts o = carve(ws, M, K, C);
    if (const int rc = launch_ab(stop, X, x_dtype, ldx, W, b, labels, M, K, C, o, s)) return rc;
    const int dw_blocks = (int)((C * K + 63) / 64);
    const int db_blocks = db ? (int)((C + 3) / 4) : 0;
    hipLaunchKernelGGL(xent16_reduce_kernel<false>, dim3((unsigned)(dw_blocks + db_blocks + 1)),
                       dim3(256), 0, s, stop, o.slab, o.R, (int)C, (int)K, o.C16, dw_blocks,
                       db_blocks, o.db_slab, o.loss_tile, o.n_tiles, 1.0 / (double)M, dW, db, loss,
                       nullptr, nullptr, nullptr, nullptr, AdamCoef{});
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

// The shared argument checks: everything that can be told without touching a
// pointer, in the order the header documents.
int check_args(const char *what, const void *X, int32_t x_dtype, int64_t ldx, int64_t M, int64_t K,
               int64_t C) {
    SGC_REQUIRE(dtype_ok(x_dtype), SGC_EINVAL,
                "%s: x_dtype %d is neither SGC_DTYPE_BF16 nor SGC_DTYPE_F16", what, (int)x_dtype);
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && ldx >= K, SGC_EINVAL,
                "%s: bad shape M=%lld K=%lld C=%lld ldx=%lld (ldx >= K)", what, (long long)M,
                (long long)K, (long long)C, (long long)ldx);
    SGC_REQUIRE(std::strcmp(linear_xent_x16_kernel_name(M, K, ldx, C, X, x_dtype), "none") != 0,
                SGC_EINVAL,
                "%s: not covered (C=%lld > 48, odd pitch %lld, 2-B-aligned base, W's image past "
                "LDS at K=%lld, or past 31-bit offsets at M=%lld)",
                what, (long long)C, (long long)ldx, (long long)K, (long long)M);
    return SGC_OK;
}

}  // namespace

const char *linear_xent_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                        const void *X, int32_t x_dtype) {
    if (std::strcmp(linear_x16_kernel_name(M, K, ldx, C, X, x_dtype), "none") == 0 ||
        std::strcmp(linear_backward_x16_kernel_name(M, K, ldx, C, X, x_dtype), "none") == 0)
        return "none";
    return x_dtype == SGC_DTYPE_BF16
               ? "xent_fwd_x16_kernel + xent_dw_cols_x16_kernel (bf16 X, v_mfma_f32_16x16x32_bf16 x 3 products)"
               : "xent_fwd_x16_kernel + xent_dw_cols_x16_kernel (fp16 X, v_mfma_f32_16x16x32_bf16 x 5 products)";
}

// G [M][C16] | loss partials [ceil(M / 16)] | dW partials [R][C16][K] | db partials [R][C16]
int64_t linear_xent_x16_workspace_bytes(int64_t M, int64_t K, int64_t C) {
    // every covered shape at its tightest layout (ldx = K rounded up to even, an aligned base)
    if (M <= 0 || K <= 0 || C <= 0 ||
        std::strcmp(linear_xent_x16_kernel_name(M, K, (K + 1) / 2 * 2, C, nullptr, SGC_DTYPE_BF16),
                    "none") == 0)
        return 0;
    const int64_t C16 = (C + 15) / 16 * 16, R = dw_cols_x16_ranges(M);
    return al256(M * C16 * 4) + al256((M + 15) / 16 * 8) + al256(R * C16 * K * 4) +
           al256(R * C16 * 4) + 512;
}

int linear_xent_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, float *loss, float *dW,
                    float *db, void *ws, int64_t ws_bytes, hipStream_t s) {
    if (const int rc = check_args("linear_xent_x16", X, x_dtype, ldx, M, K, C)) return rc;
    SGC_REQUIRE(X && W && labels && loss && dW && ws, SGC_EINVAL, "linear_xent_x16: null pointer");
    const int64_t need = linear_xent_x16_workspace_bytes(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "linear_xent_x16: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    return step_launches(nullptr, X, x_dtype, ldx, W, b, labels, M, K, C, loss, dW, db, ws, s);
}

// ---- the closure of sgc_train_lbfgs_x16 (lbfgs.hip) ----------------------------
int xent_x16_closure_check(const char *what, const void *X, int32_t x_dtype, int64_t ldx, int64_t M,
                           int64_t K, int64_t C) {
    return check_args(what, X, x_dtype, ldx, M, K, C);
}

int xent_x16_closure(const int64_t *stop, const void *X, int32_t x_dtype, int64_t ldx,
                     const float *W, const float *b, const int64_t *labels, int64_t M, int64_t K,
                     int64_t C, float *loss, float *dW, float *db, void *ws, hipStream_t s) {
    return step_launches(stop, X, x_dtype, ldx, W, b, labels, M, K, C, loss, dW, db, ws, s);
}

// ---- sgc_train_adam_x16 ---------------------------------------------------------
// sgc_train_adam_f32's general schedule on 16-bit X: per epoch launches A and B,
// then the reduction with the Adam update applied in place; the next epoch's
// launch A is stream-ordered behind it.  (The small schedule is fp32-only.)
int64_t train_adam_x16_workspace(int64_t M, int64_t K, int64_t C) {
    return linear_xent_x16_workspace_bytes(M, K, C);
}

int train_adam_x16(const void *X, int32_t x_dtype, int64_t ldx, float *W, float *b,
                   const int64_t *labels, int64_t M, int64_t K, int64_t C, float *mW, float *vW,
                   float *mb, float *vb, int64_t step0, int32_t epochs, double lr, double beta1,
                   double beta2, double eps, double weight_decay, float *loss_trace, void *ws,
                   int64_t ws_bytes, hipStream_t s) {
    SGC_REQUIRE(epochs >= 0, SGC_EINVAL, "train_adam_x16: epochs=%d < 0", epochs);
    if (const int rc = check_args("train_adam_x16", X, x_dtype, ldx, M, K, C)) return rc;
    SGC_REQUIRE(step0 >= 0, SGC_EINVAL, "train_adam_x16: step0=%lld < 0", (long long)step0);
    SGC_REQUIRE(b ? (mb && vb) : (!mb && !vb), SGC_EINVAL,
                "train_adam_x16: b and its two moments must be given or NULL together");
    SGC_REQUIRE(X && W && labels && mW && vW && ws, SGC_EINVAL, "train_adam_x16: null pointer");
    const int64_t need = train_adam_x16_workspace(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "train_adam_x16: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    if (epochs == 0) return SGC_OK;
    g_adam_kernel_last = 1;
    const Parts o = carve(ws, M, K, C);
    const int dw_blocks = (int)((C * K + 63) / 64);
    const int db_blocks = b ? (int)((C + 3) / 4) : 0;
    for (int e = 0; e < epochs; ++e) {
        const AdamCoef coef = adam_coef(step0 + e + 1, lr, beta1, beta2, eps, weight_decay);
        if (const int rc = launch_ab(nullptr, X, x_dtype, ldx, W, b, labels, M, K, C, o, s))
            return rc;
        float *loss_out = loss_trace ? loss_trace + e : nullptr;
        // (without a loss output the last block is not launched)
        hipLaunchKernelGGL(xent16_reduce_kernel<true>,
                           dim3((unsigned)(dw_blocks + db_blocks + (loss_out ? 1 : 0))), dim3(256), 0,
                           s, nullptr, o.slab, o.R, (int)C, (int)K, o.C16, dw_blocks, db_blocks,
                           o.db_slab, o.loss_tile, o.n_tiles, 1.0 / (double)M, W, b, loss_out, mW,
                           vW, mb, vb, coef);
        SGC_HIP_CHECK(hipGetLastError());
    }
    return SGC_OK;
}

}  // namespace sgc
