// lbfgs_wide.hip -- the L-BFGS iteration of lbfgs.hip for parameter vectors of
// any length, spread over the machine.
//
// lbfgs.hip keeps the vector in the registers of one workgroup and runs the
// two-loop recursion as 2 hist_len dependent dot products over it.  Here the
// recursion runs in coefficient space instead (the compact, Gram form): the
// state keeps, in fp64, every dot product between the basis vectors
// {s_i, y_i, g}.  q and r of the recursion are then coefficient vectors of
// length 2 hist_len + 1, the dependent dot products are sums over Gram rows in
// one small workgroup, and d is formed as one linear combination of the basis.
//
// One iteration is six launches, whatever n and hist_len are:
//   1 scan     (n / tile workgroups) stages s_new = t d and y_new = g - prev_g
//              outside the ring, and writes per-workgroup partials of the dots
//              of s_new, y_new and g against every ring row and one another,
//              and of max|g|, |g|_1, max|t d|
//   2 coef     (one workgroup) sums the partials in workgroup order, runs
//              torch's entry tests, accepts or rejects the pair, updates
//              the Gram block, H_diag and the step size, runs the two loops
//              on coefficients
//   3 direct   (n / tile) moves an accepted pair into its ring slot, writes
//              d = sum coef_k basis_k and prev_g = g, and the partials of g.d
//   4 decide   (one thread) the g.d test
//   5 update   (n / tile) x += t d
//   6 settle   (one thread) clears the hand-over word of 5
// Every launch of a stopped step returns at entry without a store.
//
// Arithmetic as in lbfgs.hip: fp32 vectors; every dot product, 1-norm and max
// an fp64 accumulation of exact fp32 products in a fixed order (per thread in
// element order, a xor butterfly in the wave, the four waves in order, the
// workgroup partials in workgroup order); coefficient-space sums in fp64;
// x += t d a single fmaf.  The cut of [0, n) into tiles depends on n only.
//
// The header prefix, the tensor table, torch's decisions (entry tests, pair
// acceptance), the state registry, init / begin / status and the fused
// training loop are lbfgs_common.h's, shared with lbfgs.hip; this file holds
// the six launches, the Gram maintenance, sync_gram and the L2 term.
#include <cmath>

#include "lbfgs_common.h"

namespace sgc {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr const Engine &kE = kWideEngine;
constexpr int kScalars = 16;  // leading dots of a partial block (9 used)
constexpr int kBatch = 128;   // ring rows reduced per LDS image

// partial / reduced dot slots
enum { D_GMAX = 0, D_G1, D_TDMAX, D_SS, D_SY, D_YY, D_SG, D_YG, D_GG };

struct Header : HeaderBase {
    int64_t live;       // coef -> direct, decide: this iteration passed the entry tests
    int64_t move;       // decide -> update: g.d passed; settle clears it
    int64_t pushed;     // coef -> direct: the staged pair goes into push_slot
    int64_t push_slot;
    int64_t nwg;        // tiles of the vector (tiles(ld): by n alone)
};
static_assert(sizeof(Header) == 144, "the wide words follow the shared prefix");

typedef Tensors<int64_t> Table;

// 16-B chunks per thread of a tile (tile = 1024 nv floats): by n alone
__host__ __device__ constexpr int tile_nv(int64_t ld) {
    return ld <= (int64_t)256 * 1024 ? 1 : (ld <= (int64_t)512 * 2048 ? 2 : 4);
}
__host__ __device__ constexpr int64_t tiles(int64_t ld) {
    return (ld + 1024 * tile_nv(ld) - 1) / (1024 * tile_nv(ld));
}
__host__ __device__ constexpr int64_t partial_stride(int64_t m) { return kScalars + 6 * m; }

// state: header | ro[m] | d | prev_g | S[m] | Y[m] | s_new | y_new |
//        coef[2m+1] f64 | red[16+6m] f64 | G[(2m+1)^2] f64 | partials[nwg][16+6m] f64
struct Layout {
    int64_t ro, d, pg, S, Y, s_new, y_new, coef, red, G, part, bytes;
};
__host__ __device__ inline Layout layout(int64_t n, int64_t m) {
    const int64_t ld = row_ld(n), B = 2 * m + 1;
    Layout L;
    L.ro = kHeaderBytes;
    L.d = L.ro + scalars_bytes(m);
    L.pg = L.d + ld * 4;
    L.S = L.pg + ld * 4;
    L.Y = L.S + m * ld * 4;
    L.s_new = L.Y + m * ld * 4;
    L.y_new = L.s_new + ld * 4;
    L.coef = L.y_new + ld * 4;
    L.red = L.coef + round_up(B * 8, 256);
    L.G = L.red + round_up(partial_stride(m) * 8, 256);
    L.part = L.G + round_up(B * B * 8, 256);
    L.bytes = L.part + round_up(tiles(ld) * partial_stride(m) * 8, 256);
    return L;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, kWave));
    return v;
}

template <int NV>
__device__ __forceinline__ void load_grad(const Table &T, int64_t n, int64_t nc, int64_t c0,
                                          f4 (&g)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int64_t c = c0 + kThreads * k;
        g[k] = f4{0.f, 0.f, 0.f, 0.f};
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * c + e < n) g[k][e] = flat_grad(T, 4 * c + e);
        }
    }
}

// The one dot routine of the file: this workgroup's partials of row . probe_p
// for the `rows` rows row_of(q) against NP probe vectors held in registers,
// written to out[q * NP + p].  Per thread in chunk order, the wave butterfly,
// the four wave sums in wave order.
template <int NV, int NP, typename RowOf>
__device__ __forceinline__ void scan_rows(const f4 (&probe)[NP][NV], int rows, RowOf row_of,
                                          int64_t nc, int64_t c0, double *out,
                                          double (*red)[NP][kWaves]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int q0 = 0; q0 < rows; q0 += kBatch) {
        const int qn = rows - q0 < kBatch ? rows - q0 : kBatch;
        for (int q = 0; q < qn; ++q) {
            const float *row = row_of(q0 + q);
            f4 v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = load_chunk(row, nc, c0 + kThreads * k);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < NV; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc += (double)v[k][e] * (double)probe[p][k][e];
                acc = wave_sum(acc);
                if (lane == 0) red[q][p][wave] = acc;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < qn * NP; i += kThreads) {
            const double *w = &red[0][0][0] + (int64_t)i * kWaves;
            double a = w[0];
#pragma unroll
            for (int k = 1; k < kWaves; ++k) a += w[k];
            out[(int64_t)q0 * NP + i] = a;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int ring_slot(int head, int i, int m) { return (head + i) % m; }

// ---- 1 scan ---------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(kThreads) void wide_scan_kernel(char *state, Table T) {
    __shared__ double red[kBatch][3][kWaves];
    __shared__ double sred[9][kWaves];
    const Header *H = reinterpret_cast<const Header *>(state);
    if (H->stop != 0) return;
    const int64_t n = H->n, ld = H->ld, nc = ld >> 2;
    const int m = (int)H->history_size, h = (int)H->hist_len, head = (int)H->head;
    const float t = H->t;
    const Layout L = layout(n, m);
    const float *d_g = reinterpret_cast<const float *>(state + L.d);
    const float *pg_g = reinterpret_cast<const float *>(state + L.pg);
    const float *S_g = reinterpret_cast<const float *>(state + L.S);
    const float *Y_g = reinterpret_cast<const float *>(state + L.Y);
    float *sn_g = reinterpret_cast<float *>(state + L.s_new);
    float *yn_g = reinterpret_cast<float *>(state + L.y_new);
    double *out = reinterpret_cast<double *>(state + L.part) +
                  (int64_t)blockIdx.x * partial_stride(m);
    const int64_t c0 = (int64_t)blockIdx.x * (kThreads * NV) + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;

    f4 probe[3][NV];  // s_new, y_new, g
    load_grad<NV>(T, n, nc, c0, probe[2]);
    double r[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int64_t c = c0 + kThreads * k;
        const f4 pg = load_chunk(pg_g, nc, c), d = load_chunk(d_g, nc, c);
        const f4 g = probe[2][k];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double ag = fabs((double)g[e]);
            r[D_GMAX] = nan_max(r[D_GMAX], ag);
            r[D_G1] += ag;
            r[D_TDMAX] = nan_max(r[D_TDMAX], fabs((double)t * (double)d[e]));
            const float y = g[e] - pg[e], s = d[e] * t;
            probe[0][k][e] = s;
            probe[1][k][e] = y;
            r[D_SS] += (double)s * (double)s;
            r[D_SY] += (double)s * (double)y;
            r[D_YY] += (double)y * (double)y;
            r[D_SG] += (double)s * (double)g[e];
            r[D_YG] += (double)y * (double)g[e];
            r[D_GG] += (double)g[e] * (double)g[e];
        }
        if (c < nc) {
            reinterpret_cast<f4 *>(sn_g)[c] = probe[0][k];
            reinterpret_cast<f4 *>(yn_g)[c] = probe[1][k];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const bool mx = i == D_GMAX || i == D_TDMAX;
        r[i] = mx ? wave_max(r[i]) : wave_sum(r[i]);
        if (lane == 0) sred[i][wave] = r[i];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int i = threadIdx.x;
        const bool mx = i == D_GMAX || i == D_TDMAX;
        double a = sred[i][0];
        for (int k = 1; k < kWaves; ++k) a = mx ? nan_max(a, sred[i][k]) : a + sred[i][k];
        out[i] = a;
    }
    // ring rows in logical order, S then Y of each pair
    auto row_of = [&](int q) {
        const int sl = ring_slot(head, q >> 1, m);
        return ((q & 1) ? Y_g : S_g) + (int64_t)sl * ld;
    };
    scan_rows<NV, 3>(probe, 2 * h, row_of, nc, c0, out + kScalars, red);
}

// the partials of dot `id` over the workgroups, in workgroup order
__device__ __forceinline__ double sum_partials(const double *part, int64_t stride, int64_t nwg,
                                               int64_t id, bool mx) {
    double a = 0.0;
    for (int64_t w = 0; w < nwg; ++w) {
        const double v = part[w * stride + id];
        a = mx ? nan_max(a, v) : a + v;
    }
    return a;
}

// ---- 2 coef ---------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wide_coef_kernel(char *state,
                                                             const float *__restrict__ loss_ptr,
                                                             float lr, int max_eval,
                                                             double tol_grad, double tol_change) {
    __shared__ double c_s[2 * kMaxHistory + 1];
    __shared__ double al_s[kMaxHistory];
    __shared__ int idx_s[2 * kMaxHistory + 1];
    Header *H = reinterpret_cast<Header *>(state);
    if (H->stop != 0) return;
    const int tid = threadIdx.x;
    const int64_t n = H->n;
    const int m = (int)H->history_size;
    const Layout L = layout(n, m);
    const int64_t nwg = H->nwg, P = partial_stride(m), B = 2 * m + 1;
    int n_iter = (int)H->n_iter, func_evals = (int)H->func_evals;
    int iters = (int)H->iters, evals = (int)H->evals;
    int h = (int)H->hist_len, head = (int)H->head;
    float H_diag = H->H_diag;
    const double prev_loss = H->prev_loss;
    float *ro_g = reinterpret_cast<float *>(state + L.ro);
    double *coef = reinterpret_cast<double *>(state + L.coef);
    double *red = reinterpret_cast<double *>(state + L.red);
    double *G = reinterpret_cast<double *>(state + L.G);
    const double *part = reinterpret_cast<const double *>(state + L.part);
    const double loss = (double)*loss_ptr;

    const int h_old = h, head_old = head;
    for (int id = tid; id < kScalars + 6 * h_old; id += kThreads)
        red[id] = sum_partials(part, P, nwg, id, id == D_GMAX || id == D_TDMAX);
    __syncthreads();

    const double gmax = red[D_GMAX];
    int stop = 0;
    func_evals += 1;
    evals += 1;
    stop = entry_stop(evals, max_eval, gmax, red[D_TDMAX], loss, prev_loss, tol_grad, tol_change);
    if (stop != 0) {
        if (tid == 0) {
            H->func_evals = func_evals;
            H->evals = evals;
            H->stop = stop;
            H->loss = loss;
        }
        return;
    }
    n_iter += 1;
    iters += 1;
    const float g1 = (float)red[D_G1], ys = (float)red[D_SY], yy = (float)red[D_YY];
    const bool first = n_iter == 1;
    const PairDecision D = accept_pair(first, ys, yy, m, head, h, H_diag, [](int) {});
    const bool push = D.push, evict = D.evict;
    const int slot = D.slot;
    head = D.head;
    h = D.hist_len;
    H_diag = D.H_diag;
    const float t = step_size(first, g1, lr);

    // the Gram block: the pair's row and column (when accepted) and g's
    const int64_t ig = 2 * m;
    for (int q = tid; q < 2 * h_old; q += kThreads) {
        const int i = q >> 1;
        if (evict && i == 0) continue;  // the pair that leaves
        const int sl = ring_slot(head_old, i, m);
        const int64_t R = (q & 1) ? m + sl : sl;
        const double *dq = red + kScalars + 3 * q;
        if (push) {
            G[slot * B + R] = G[R * B + slot] = dq[0];
            G[(m + slot) * B + R] = G[R * B + (m + slot)] = dq[1];
        }
        G[ig * B + R] = G[R * B + ig] = dq[2];
    }
    if (tid == 0) {
        if (push) {
            G[slot * B + slot] = red[D_SS];
            G[slot * B + (m + slot)] = G[(m + slot) * B + slot] = red[D_SY];
            G[(m + slot) * B + (m + slot)] = red[D_YY];
            G[ig * B + slot] = G[slot * B + ig] = red[D_SG];
            G[ig * B + (m + slot)] = G[(m + slot) * B + ig] = red[D_YG];
            ro_g[slot] = 1.0f / ys;
        }
        G[ig * B + ig] = red[D_GG];
    }
    // the coefficient vector over (s_0 .. s_h-1, y_0 .. y_h-1, g), logical order
    const int nb = 2 * h + 1;
    for (int e = tid; e < nb; e += kThreads) {
        idx_s[e] = e < h ? ring_slot(head, e, m) : (e < 2 * h ? m + ring_slot(head, e - h, m) : 2 * m);
        c_s[e] = e == 2 * h ? -1.0 : 0.0;
    }
    __syncthreads();

    // the two loops, one wave: the dot of a Gram row with the coefficients is
    // lane-strided over the entries and a butterfly, so every lane holds it
    if (tid < kWave) {
        const int lane = tid;
        for (int i = h - 1; i >= 0; --i) {
            const int sl = ring_slot(head, i, m);
            const double *row = G + (int64_t)sl * B;
            double a = 0.0;
            for (int e = lane; e < nb; e += kWave) a += c_s[e] * row[idx_s[e]];
            a = wave_sum(a);
            const double al = a * (double)ro_g[sl];
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                al_s[i] = al;
                c_s[h + i] -= al;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        for (int e = lane; e < nb; e += kWave) c_s[e] *= (double)H_diag;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < h; ++i) {
            const int sl = ring_slot(head, i, m);
            const double *row = G + (int64_t)(m + sl) * B;
            double a = 0.0;
            for (int e = lane; e < nb; e += kWave) a += c_s[e] * row[idx_s[e]];
            a = wave_sum(a);
            const double be = a * (double)ro_g[sl];
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) c_s[i] += al_s[i] - be;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        for (int e = lane; e < nb; e += kWave) coef[e] = c_s[e];
        if (lane == 0) {
            H->n_iter = n_iter;
            H->func_evals = func_evals;
            H->iters = iters;
            H->evals = evals;
            H->hist_len = h;
            H->head = head;
            H->loss = loss;
            H->prev_loss = loss;
            H->H_diag = H_diag;
            H->t = t;
            H->pushed = push ? 1 : 0;
            H->push_slot = slot;
            H->live = 1;
        }
    }
}

// ---- 3 direct -------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(kThreads) void wide_direct_kernel(char *state, Table T) {
    __shared__ double c_s[2 * kMaxHistory + 1];
    __shared__ double wred[kWaves];
    const Header *H = reinterpret_cast<const Header *>(state);
    if (H->live == 0) return;
    const int64_t n = H->n, ld = H->ld, nc = ld >> 2;
    const int m = (int)H->history_size, h = (int)H->hist_len, head = (int)H->head;
    const bool pushed = H->pushed != 0;
    const int pslot = (int)H->push_slot;
    const Layout L = layout(n, m);
    float *d_g = reinterpret_cast<float *>(state + L.d);
    float *pg_g = reinterpret_cast<float *>(state + L.pg);
    float *S_g = reinterpret_cast<float *>(state + L.S);
    float *Y_g = reinterpret_cast<float *>(state + L.Y);
    const float *sn_g = reinterpret_cast<const float *>(state + L.s_new);
    const float *yn_g = reinterpret_cast<const float *>(state + L.y_new);
    const double *coef = reinterpret_cast<const double *>(state + L.coef);
    double *out = reinterpret_cast<double *>(state + L.part) +
                  (int64_t)blockIdx.x * partial_stride(m);
    const int64_t c0 = (int64_t)blockIdx.x * (kThreads * NV) + threadIdx.x;
    for (int e = threadIdx.x; e < 2 * h + 1; e += kThreads) c_s[e] = coef[e];
    __syncthreads();

    f4 sn[NV], yn[NV], g[NV];
    double acc[NV][4];
    load_grad<NV>(T, n, nc, c0, g);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int64_t c = c0 + kThreads * k;
        sn[k] = load_chunk(sn_g, nc, c);
        yn[k] = load_chunk(yn_g, nc, c);
        if (pushed && c < nc) {
            reinterpret_cast<f4 *>(S_g + (int64_t)pslot * ld)[c] = sn[k];
            reinterpret_cast<f4 *>(Y_g + (int64_t)pslot * ld)[c] = yn[k];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.0;
    }
    // d = sum coef_k basis_k per element, in the coefficients' order
    for (int q = 0; q < 2 * h; ++q) {
        const int sl = ring_slot(head, q < h ? q : q - h, m);
        const bool staged = pushed && sl == pslot;
        const float *row = (q < h ? S_g : Y_g) + (int64_t)sl * ld;
        const double cq = c_s[q];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const f4 v = staged ? (q < h ? sn[k] : yn[k]) : load_chunk(row, nc, c0 + kThreads * k);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] = fma(cq, (double)v[e], acc[k][e]);
        }
    }
    const double cg = c_s[2 * h];
    double gd = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int64_t c = c0 + kThreads * k;
        f4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d[e] = 4 * c + e < n ? (float)fma(cg, (double)g[k][e], acc[k][e]) : 0.0f;
            gd += (double)g[k][e] * (double)d[e];
        }
        if (c < nc) {
            reinterpret_cast<f4 *>(d_g)[c] = d;
            reinterpret_cast<f4 *>(pg_g)[c] = g[k];
        }
    }
    gd = wave_sum(gd);
    if ((threadIdx.x & (kWave - 1)) == 0) wred[threadIdx.x / kWave] = gd;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = wred[0];
        for (int k = 1; k < kWaves; ++k) a += wred[k];
        out[0] = a;
    }
}

// ---- 4 decide, 6 settle ---------------------------------------------------------
__global__ void wide_decide_kernel(char *state, int max_iter, double tol_change) {
    Header *H = reinterpret_cast<Header *>(state);
    if (H->live == 0) return;
    const Layout L = layout(H->n, H->history_size);
    const double *part = reinterpret_cast<const double *>(state + L.part);
    const float gtd =
        (float)sum_partials(part, partial_stride(H->history_size), H->nwg, 0, false);
    H->live = 0;
    if ((double)gtd > -tol_change) {
        H->stop = SGC_LBFGS_STOP_GTD;  // the parameters stay where they are
    } else {
        H->move = 1;
        if (H->iters >= max_iter) H->stop = SGC_LBFGS_STOP_MAX_ITER;
    }
}

__global__ void wide_settle_kernel(Header *H) {
    if (H->move != 0) H->move = 0;
}

// ---- 5 update -------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(kThreads) void wide_update_kernel(const char *state, Table T) {
    const Header *H = reinterpret_cast<const Header *>(state);
    if (H->move == 0) return;
    const int64_t n = H->n, nc = H->ld >> 2;
    const float t = H->t;
    const Layout L = layout(n, H->history_size);
    const float *d_g = reinterpret_cast<const float *>(state + L.d);
    const int64_t c0 = (int64_t)blockIdx.x * (kThreads * NV) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int64_t c = c0 + kThreads * k;
        if (c >= nc) continue;
        const f4 d = reinterpret_cast<const f4 *>(d_g)[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = 4 * c + e;
            if (j >= n) continue;
            update_param(T, j, t, d, e);
        }
    }
}

// ---- sync_gram: one basis row against every row ------------------------------------
// basis index a: S slot a, Y slot a - m, 2m = prev_g (the g of the last iteration)
__device__ __forceinline__ const float *basis_row(const char *state, const Layout &L, int64_t ld,
                                                  int m, int a) {
    if (a == 2 * m) return reinterpret_cast<const float *>(state + L.pg);
    return reinterpret_cast<const float *>(state + (a < m ? L.S : L.Y)) +
           (int64_t)(a < m ? a : a - m) * ld;
}

template <int NV>
__global__ __launch_bounds__(kThreads) void wide_gram_scan_kernel(char *state, int a) {
    __shared__ double red[kBatch][1][kWaves];
    const Header *H = reinterpret_cast<const Header *>(state);
    const int64_t n = H->n, ld = H->ld, nc = ld >> 2;
    const int m = (int)H->history_size;
    const Layout L = layout(n, m);
    const int64_t c0 = (int64_t)blockIdx.x * (kThreads * NV) + threadIdx.x;
    // (2m + 1 <= 16 + 6m: a partial block holds one dot per basis row)
    double *out = reinterpret_cast<double *>(state + L.part) +
                  (int64_t)blockIdx.x * partial_stride(m);
    f4 probe[1][NV];
    const float *pa = basis_row(state, L, ld, m, a);
#pragma unroll
    for (int k = 0; k < NV; ++k) probe[0][k] = load_chunk(pa, nc, c0 + kThreads * k);
    auto row_of = [&](int q) { return basis_row(state, L, ld, m, q); };
    scan_rows<NV, 1>(probe, 2 * m + 1, row_of, nc, c0, out, red);
}

__global__ __launch_bounds__(kThreads) void wide_gram_row_kernel(char *state, int a) {
    const Header *H = reinterpret_cast<const Header *>(state);
    const int m = (int)H->history_size;
    const Layout L = layout(H->n, m);
    const int64_t B = 2 * m + 1;
    double *G = reinterpret_cast<double *>(state + L.G);
    const double *part = reinterpret_cast<const double *>(state + L.part);
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q < B) G[(int64_t)a * B + q] = sum_partials(part, partial_stride(m), H->nwg, q, false);
}

// ---- the L2 term of the reference's closure, behind the stop word ------------------
constexpr int kL2Tile = 4096;

// g_W += l2 W (one fmaf each) and this tile's fp64 partial of sum W^2
__global__ __launch_bounds__(kThreads) void wide_l2_grad_kernel(const int64_t *stop,
                                                                const float *__restrict__ W,
                                                                float *__restrict__ gW, int64_t n,
                                                                float l2, double *part) {
    __shared__ double wred[kWaves];
    if (*stop != 0) return;
    const int64_t base = (int64_t)blockIdx.x * kL2Tile;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < kL2Tile / kThreads; ++k) {
        const int64_t j = base + threadIdx.x + kThreads * k;
        if (j < n) {
            const float w = W[j];
            gW[j] = fmaf(l2, w, gW[j]);
            acc += (double)w * (double)w;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) wred[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = wred[0];
        for (int k = 1; k < kWaves; ++k) a += wred[k];
        part[blockIdx.x] = a;
    }
}

// loss += 0.5 l2 sum W^2: the partials in tile order, rounded once, one fp32 add
__global__ void wide_l2_loss_kernel(const int64_t *stop, const double *part, int64_t nt, double l2,
                                    float *loss) {
    if (*stop != 0) return;
    double a = 0.0;
    for (int64_t i = 0; i < nt; ++i) a += part[i];
    *loss = *loss + (float)(0.5 * l2 * a);
}

#define WIDE_LAUNCH_NV(kernel, nv, grid, s, ...)                                              \
    do {                                                                                      \
        if ((nv) == 1) hipLaunchKernelGGL(kernel<1>, grid, dim3(kThreads), 0, s, __VA_ARGS__); \
        else if ((nv) == 2)                                                                   \
            hipLaunchKernelGGL(kernel<2>, grid, dim3(kThreads), 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL(kernel<4>, grid, dim3(kThreads), 0, s, __VA_ARGS__);          \
    } while (0)

// the six launches of one iteration
hipError_t enqueue_iterate(char *st, const Table &T, int64_t n, const float *loss, float lrf,
                           int max_iter, int max_eval, double tol_grad, double tol_change,
                           hipStream_t s) {
    const int64_t ld = row_ld(n);
    const int nv = tile_nv(ld);
    const dim3 grid((unsigned)tiles(ld));
    WIDE_LAUNCH_NV(wide_scan_kernel, nv, grid, s, st, T);
    hipLaunchKernelGGL(wide_coef_kernel, dim3(1), dim3(kThreads), 0, s, st, loss, lrf, max_eval,
                       tol_grad, tol_change);
    WIDE_LAUNCH_NV(wide_direct_kernel, nv, grid, s, st, T);
    hipLaunchKernelGGL(wide_decide_kernel, dim3(1), dim3(1), 0, s, st, max_iter, tol_change);
    WIDE_LAUNCH_NV(wide_update_kernel, nv, grid, s, (const char *)st, T);
    hipLaunchKernelGGL(wide_settle_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<Header *>(st));
    return hipGetLastError();
}

// the two launches of the L2 term (partials: the state's partial region, which
// holds at least one double per 1024 floats of the vector)
hipError_t enqueue_l2(char *st, const StateShape &sh, const float *W, float *gW, int64_t ck,
                      double l2, float *loss, hipStream_t s) {
    const int64_t *stop = &reinterpret_cast<const Header *>(st)->stop;
    double *part = reinterpret_cast<double *>(st + layout(sh.n, sh.m).part);
    const int64_t nt = (ck + kL2Tile - 1) / kL2Tile;
    hipLaunchKernelGGL(wide_l2_grad_kernel, dim3((unsigned)nt), dim3(kThreads), 0, s, stop, W, gW,
                       ck, (float)l2, part);
    hipLaunchKernelGGL(wide_l2_loss_kernel, dim3(1), dim3(1), 0, s, stop, (const double *)part, nt,
                       l2, loss);
    return hipGetLastError();
}

}  // namespace

int64_t lbfgs_wide_workspace(int64_t n, int32_t history_size) {
    if (check_shape("lbfgs_wide_workspace", n, history_size, kE)) return 0;
    return layout(n, history_size).bytes;
}

int lbfgs_wide_init(void *state, int64_t bytes, int64_t n, int32_t history_size, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_wide_init: null state");
    if (const int rc = check_shape("lbfgs_wide_init", n, history_size, kE)) return rc;
    return state_init("lbfgs_wide_init", kE, state, bytes, layout(n, history_size).bytes, n,
                      history_size, &reinterpret_cast<Header *>(state)->nwg, tiles(row_ld(n)), s);
}

int lbfgs_wide_iterate(void *state, int32_t n_tensors, float *const *params,
                       const float *const *grads, const int64_t *numels, const float *loss,
                       double lr, int32_t max_iter, int32_t max_eval, double tol_grad,
                       double tol_change, hipStream_t s) {
    return iterate_entry<int64_t>("lbfgs_wide_iterate", kE, enqueue_iterate, state, n_tensors,
                                  params, grads, numels, loss, lr, max_iter, max_eval, tol_grad,
                                  tol_change, s);
}

int lbfgs_wide_sync_gram(void *state, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_wide_sync_gram: null state");
    StateShape sh;
    if (const int rc = find_state("lbfgs_wide_sync_gram", state, kE, sh)) return rc;
    const int64_t ld = row_ld(sh.n);
    const int nv = tile_nv(ld);
    const dim3 grid((unsigned)tiles(ld));
    const int B = 2 * (int)sh.m + 1;
    char *st = reinterpret_cast<char *>(state);
    for (int a = 0; a < B; ++a) {
        WIDE_LAUNCH_NV(wide_gram_scan_kernel, nv, grid, s, st, a);
        hipLaunchKernelGGL(wide_gram_row_kernel, dim3((B + kThreads - 1) / kThreads),
                           dim3(kThreads), 0, s, st, a);
    }
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

int lbfgs_wide_l2(void *state, const float *W, float *gW, int64_t numel, double l2, float *loss,
                  hipStream_t s) {
    SGC_REQUIRE(state && W && gW && loss, SGC_EINVAL, "lbfgs_wide_l2: null pointer");
    StateShape sh;
    if (const int rc = find_state("lbfgs_wide_l2", state, kE, sh)) return rc;
    SGC_REQUIRE(numel >= 1 && numel <= sh.n, SGC_EINVAL,
                "lbfgs_wide_l2: numel=%lld outside 1..n=%lld", (long long)numel, (long long)sh.n);
    if (l2 == 0.0) return SGC_OK;
    const hipError_t e = enqueue_l2(reinterpret_cast<char *>(state), sh, W, gW, numel, l2, loss, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "lbfgs_wide_l2 launch failed: %s",
                hipGetErrorString(e));
    return SGC_OK;
}

// ---- sgc_train_lbfgs_wide_f32: run_train_steps (lbfgs_common.h) on the wide
// iteration; the closure is xent_closure behind the state's stop word, then the
// L2 term when l2 != 0 ----------------------------------------------------------------
int64_t train_lbfgs_wide_workspace(int64_t M, int64_t K, int64_t C) {
    if (M <= 0 || K <= 0 || C <= 0 || C > 64 || C * K + C >= INT32_MAX) return 0;
    return train_workspace_bytes(K, C, xent_workspace_bytes(M, K, C));
}

int train_lbfgs_wide(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                     int64_t M, int64_t K, int64_t C, void *state, int32_t steps, double lr,
                     int32_t max_iter, int32_t max_eval, double tol_grad, double tol_change,
                     double l2, float *loss_trace, int64_t *status_trace, void *ws,
                     int64_t ws_bytes, hipStream_t s) {
    const char *what = "train_lbfgs_wide";
    SGC_REQUIRE(steps >= 0, SGC_EINVAL, "%s: steps=%d < 0", what, steps);
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && C <= 64 && ldx >= K, SGC_EINVAL,
                "%s: bad shape M=%lld K=%lld C=%lld ldx=%lld (1 <= C <= 64, ldx >= K)", what,
                (long long)M, (long long)K, (long long)C, (long long)ldx);
    SGC_REQUIRE(max_iter >= 1, SGC_EINVAL, "%s: max_iter=%d < 1", what, max_iter);
    SGC_REQUIRE(X && W && labels && state && ws, SGC_EINVAL, "%s: null pointer", what);
    SGC_REQUIRE(reinterpret_cast<uintptr_t>(X) % 4 == 0, SGC_EINVAL, "%s: X not 4-B aligned",
                what);
    const int64_t ck = C * K, n = ck + (b ? C : 0);
    SGC_REQUIRE(ck + C < INT32_MAX, SGC_ERANGE, "%s: n=%lld >= 2^31 - 1 parameters", what,
                (long long)n);
    if (const int rc = xent_closure_check(what, M, K, C, ldx)) return rc;
    const int64_t need = train_lbfgs_wide_workspace(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "%s: workspace %lld < %lld", what,
                (long long)ws_bytes, (long long)need);
    if (steps == 0) return SGC_OK;
    char *st = reinterpret_cast<char *>(state);
    auto closure = [&](const StateShape &sh, const int64_t *stop, float *loss, float *dW,
                       float *db, void *xent_ws) -> int {
        if (const int rc =
                xent_closure(stop, X, ldx, W, b, labels, M, K, C, loss, dW, db, xent_ws, s))
            return rc;
        if (l2 == 0.0) return SGC_OK;
        const hipError_t e = enqueue_l2(st, sh, W, dW, ck, l2, loss, s);
        SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
        return SGC_OK;
    };
    return run_train_steps<int64_t>(what, kE, closure, enqueue_iterate, W, b, K, C, state, steps,
                                    lr, max_iter, max_eval, tol_grad, tol_change, loss_trace,
                                    status_trace, ws, s);
}

SGC_WARM_UNIT(warm_lbfgs_wide)

}  // namespace sgc
