// lbfgs.hip -- one L-BFGS iteration per launch on gfx950: what
// torch.optim.LBFGS.step (line_search_fn=None; reddit.py:51-64) does between
// two closure calls, with no host round trip.
//
// torch's loop is   closure -> [direction, step, update, closure, tests]*
// and synchronises with the host on every dot product and every test.  Here
// the loop is cut at the closure boundary instead: after every closure the
// host enqueues lbfgs_iterate_kernel, which first runs the termination tests
// of the iteration just taken (they need the new loss and gradient), then --
// unless the step has stopped -- the memory update, the two-loop recursion,
// the step size and the in-place parameter update of the next iteration.  A
// device `stop` word makes every later launch of the step a no-op, so the
// host may enqueue max_iter closures blindly and read the status once.
//
// The parameter vector is small (Reddit 24,723 floats, at most 65,536), so
// one 1024-thread workgroup holds q / r of the recursion in registers:
// thread t owns the 16-B chunks t, t + 1024, ... of the flat vector (NV of
// them, a template parameter).  History rows are 128-B aligned (ld = n
// rounded up to 32 floats, pad columns kept zero) and read with 16-B lanes;
// parameters and gradients are separate tensors at arbitrary offsets of the
// flat vector and are read and written element by element.
//
// Arithmetic contract: vectors are fp32; every dot product, |g|_1, max|g| and
// max|t d| is accumulated in fp64 from exact products of the fp32 elements
// (per thread in chunk order, a xor butterfly inside the wave, the 16 wave
// sums in wave order) and rounded to fp32 once; elementwise updates are
// single fmafs.  Results are bitwise reproducible run to run; tolerance-equal
// to torch, not bit-equal (torch sums in fp32 in another order).
// torch's decisions (the termination tests, the acceptance of a pair, the NaN
// conventions) are lbfgs_common.h's, shared with lbfgs_wide.hip.
//
// This file holds that kernel with its entries, and the definitions of what
// lbfgs_common.h declares for both engines: the three one-thread kernels
// (init, begin, snapshot) with the calls that launch them.
#include <cmath>

#include "lbfgs_common.h"

namespace sgc {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr const Engine &kE = kNarrowEngine;
constexpr int64_t kMaxN = kE.max_n;  // 64 register elements per thread

struct Header : HeaderBase {};
typedef Tensors<int32_t> Table;  // 32-bit offsets and indices throughout

// state: header | ro[m] | d[ld] | prev_g[ld] | S[m][ld] | Y[m][ld]
int64_t state_bytes(int64_t n, int64_t m) {
    return kHeaderBytes + scalars_bytes(m) + (2 + 2 * m) * row_ld(n) * 4;
}

// a value every lane holds, moved to a scalar register
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// Sums (or NaN-keeping maxima, bit i of MAXMASK) of N doubles over the
// workgroup, the result in every thread, in a fixed order: a xor butterfly
// inside each wave, then the 16 wave partials through LDS and a 16-lane
// butterfly (lane l takes partial l & 15, so every lane ends with the same
// bits).  One barrier per call: the LDS partials alternate between two
// images, and a thread can write image p again only after the barrier of the
// call in between, which every thread reaches after its reads of image p.
template <int N, unsigned MAXMASK>
__device__ __forceinline__ void block_reduce(double (&v)[N], double (*red)[5][kWaves],
                                             int &phase) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const double w = __shfl_xor(v[i], o, kWave);
            v[i] = (MAXMASK >> i & 1u) ? nan_max(v[i], w) : v[i] + w;
        }
        if (lane == 0) red[phase][i][wave] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double a = red[phase][i][lane & (kWaves - 1)];
#pragma unroll
        for (int o = kWaves / 2; o > 0; o >>= 1) {
            const double w = __shfl_xor(a, o, kWave);
            a = (MAXMASK >> i & 1u) ? nan_max(a, w) : a + w;
        }
        v[i] = a;
    }
    phase ^= 1;
}

template <int NV>
__device__ __forceinline__ void load_row(const float *row, int nc, f4 (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = load_chunk<int>(row, nc, threadIdx.x + kThreads * k);
}

template <int NV>
__device__ __forceinline__ void store_row(float *row, int nc, const f4 (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = threadIdx.x + kThreads * k;
        if (c < nc) reinterpret_cast<f4 *>(row)[c] = v[k];
    }
}

__device__ __forceinline__ void dot_chunk(double &acc, const f4 &a, const f4 &b) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)a[e] * (double)b[e];
}

// this thread's part of row . q, the row in registers / streamed from memory
// (the same chunk order, so the same bits)
template <int NV>
__device__ __forceinline__ double dot_regs(const f4 (&a)[NV], const f4 (&q)[NV]) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) dot_chunk(acc, a[k], q[k]);
    return acc;
}

template <int NV>
__device__ __forceinline__ double dot_stream(const float *row, int nc, const f4 (&q)[NV]) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        dot_chunk(acc, load_chunk<int>(row, nc, threadIdx.x + kThreads * k), q[k]);
    return acc;
}

// q += coef * row
template <int NV>
__device__ __forceinline__ void axpy_regs(float coef, const f4 (&a)[NV], f4 (&q)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[k][e] = fmaf(coef, a[k][e], q[k][e]);
}

template <int NV>
__device__ __forceinline__ void axpy_stream(float coef, const float *row, int nc, f4 (&q)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const f4 a = load_chunk<int>(row, nc, threadIdx.x + kThreads * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[k][e] = fmaf(coef, a[e], q[k][e]);
    }
}

// NV 16-B chunks per thread.  What stays in registers across a reduction's
// barrier besides q: the next S row and the Y row of the pair up to NV = 4
// (their loads do not wait for the reduction), nothing above it, where the
// rows are streamed through (q alone is 32 / 64 registers of the 128 a wave
// of a 1024-thread workgroup has).
template <int NV>
__global__ __launch_bounds__(kThreads) void lbfgs_iterate_kernel(
    char *state, Table T, const float *__restrict__ loss_ptr, float lr, int max_iter,
    int max_eval, double tol_grad, double tol_change) {
    constexpr bool kKeepY = NV <= 4, kKeepS = NV <= 4;
    __shared__ double red[2][5][kWaves];
    __shared__ float ro_s[kMaxHistory], al_s[kMaxHistory];
    Header *H = reinterpret_cast<Header *>(state);
    if (H->stop != 0) return;  // the step has stopped: nothing moves any more
    const int tid = threadIdx.x;
    // the scalar block, wave-uniform (every thread reads it before the first
    // barrier; thread 0 writes it back after the last)
    int n_iter = uni((int)H->n_iter), func_evals = uni((int)H->func_evals);
    int iters = uni((int)H->iters), evals = uni((int)H->evals);
    int hist_len = uni((int)H->hist_len), head = uni((int)H->head);
    const int n = uni((int)H->n), m = uni((int)H->history_size), ld = uni((int)H->ld);
    const int nc = ld >> 2;
    float t = uni(H->t), H_diag = uni(H->H_diag);
    int stop = 0;
    float *ro_g = reinterpret_cast<float *>(state + kHeaderBytes);
    float *d_g = reinterpret_cast<float *>(state + kHeaderBytes + scalars_bytes(m));
    float *pg_g = d_g + ld;
    float *S_g = pg_g + ld;
    float *Y_g = S_g + (int64_t)m * ld;
    int phase = 0;

    for (int i = tid; i < m; i += kThreads) ro_s[i] = ro_g[i];
    const double loss = (double)*loss_ptr;

    // the closure's gradient, and in the same reduction everything the tests
    // and the memory update need of it: max|g|, |g|_1, max|t d|, y.s, y.y
    // with y = g - prev_g, s = t d (both zero vectors before the first
    // iteration; the sums are then unused)
    f4 q[NV];
    {
        double r[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = tid + kThreads * k;
            f4 g = {0.f, 0.f, 0.f, 0.f};
            if (c < nc) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * c + e < n) g[e] = flat_grad(T, 4 * c + e);
            }
            const f4 pg = load_chunk<int>(pg_g, nc, c), d = load_chunk<int>(d_g, nc, c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double ag = fabs((double)g[e]);
                r[0] = nan_max(r[0], ag);
                r[1] += ag;
                r[2] = nan_max(r[2], fabs((double)t * (double)d[e]));
                const float y = g[e] - pg[e], s = d[e] * t;
                r[3] += (double)y * (double)s;
                r[4] += (double)y * (double)y;
            }
            q[k] = g;
        }
        block_reduce<5, 0x5u>(r, red, phase);
        const double gmax = r[0];
        func_evals += 1;
        evals += 1;
        stop = entry_stop(evals, max_eval, gmax, r[2], loss, H->prev_loss, tol_grad, tol_change);
        if (stop != 0) {
            // (every thread read prev_loss above; the barrier orders that
            // before thread 0's writes)
            __syncthreads();
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
        const float g1 = (float)r[1], ys = (float)r[3], yy = (float)r[4];
        const bool first = n_iter == 1;
        const PairDecision D = accept_pair(first, ys, yy, m, head, hist_len, H_diag, [&](int sl) {
            if (tid == 0) ro_g[sl] = ro_s[sl] = 1.0f / ys;
        });
        const bool push = D.push;
        const int slot = D.slot;
        head = D.head;
        hist_len = D.hist_len;
        H_diag = D.H_diag;
        // y, s into the ring (recomputed: nothing but q stays in registers),
        // prev_g = g, q = -g
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = tid + kThreads * k;
            if (c < nc) {
                if (push) {
                    const f4 pg = reinterpret_cast<const f4 *>(pg_g)[c];
                    const f4 d = reinterpret_cast<const f4 *>(d_g)[c];
                    reinterpret_cast<f4 *>(Y_g + (int64_t)slot * ld)[c] = q[k] - pg;
                    reinterpret_cast<f4 *>(S_g + (int64_t)slot * ld)[c] = d * t;
                }
                reinterpret_cast<f4 *>(pg_g)[c] = q[k];
            }
            q[k] = -q[k];
        }
        t = step_size(first, g1, lr);
    }

    // two-loop recursion over the ring, logical index 0 = oldest (a thread
    // reads back only chunks it wrote itself, so the pair just pushed needs
    // no fence)
    if (n_iter > 1) {
        f4 s[kKeepS ? NV : 1], y[kKeepY ? NV : 1];
        if constexpr (kKeepS)
            if (hist_len > 0) load_row<NV>(S_g + (int64_t)((head + hist_len - 1) % m) * ld, nc, s);
        for (int i = hist_len - 1; i >= 0; --i) {
            const int sl = (head + i) % m;
            const float *yrow = Y_g + (int64_t)sl * ld;
            if constexpr (kKeepY) load_row<NV>(yrow, nc, y);  // in flight across the barrier
            double a[1];
            if constexpr (kKeepS) {
                a[0] = dot_regs<NV>(s, q);
                if (i > 0) load_row<NV>(S_g + (int64_t)((head + i - 1) % m) * ld, nc, s);
            } else {
                a[0] = dot_stream<NV>(S_g + (int64_t)sl * ld, nc, q);
            }
            block_reduce<1, 0u>(a, red, phase);
            const float al = (float)a[0] * ro_s[sl];
            if (tid == 0) al_s[i] = al;
            if constexpr (kKeepY) axpy_regs<NV>(-al, y, q);
            else axpy_stream<NV>(-al, yrow, nc, q);
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) q[k] = q[k] * H_diag;
        // forward: the roles of S and Y swap (y is kept where s was)
        if constexpr (kKeepS)
            if (hist_len > 0) load_row<NV>(Y_g + (int64_t)(head % m) * ld, nc, s);
        for (int i = 0; i < hist_len; ++i) {
            const int sl = (head + i) % m;
            const float *srow = S_g + (int64_t)sl * ld;
            if constexpr (kKeepY) load_row<NV>(srow, nc, y);
            double a[1];
            if constexpr (kKeepS) {
                a[0] = dot_regs<NV>(s, q);
                if (i + 1 < hist_len) load_row<NV>(Y_g + (int64_t)((head + i + 1) % m) * ld, nc, s);
            } else {
                a[0] = dot_stream<NV>(Y_g + (int64_t)sl * ld, nc, q);
            }
            block_reduce<1, 0u>(a, red, phase);
            const float coef = al_s[i] - (float)a[0] * ro_s[sl];
            if constexpr (kKeepY) axpy_regs<NV>(coef, y, q);
            else axpy_stream<NV>(coef, srow, nc, q);
        }
    }
    store_row<NV>(d_g, nc, q);  // d

    // directional derivative g.d (g read back from prev_g), then the update
    {
        double a[1] = {dot_stream<NV>(pg_g, nc, q)};
        block_reduce<1, 0u>(a, red, phase);
        const float gtd = (float)a[0];
        if ((double)gtd > -tol_change) {
            stop = SGC_LBFGS_STOP_GTD;  // the parameters stay where they are
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int c = tid + kThreads * k;
                if (c >= nc) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * c + e;
                    if (j >= n) continue;
                    update_param(T, j, t, q[k], e);
                }
            }
            if (iters >= max_iter) stop = SGC_LBFGS_STOP_MAX_ITER;
        }
    }
    if (tid == 0) {
        H->n_iter = n_iter;
        H->func_evals = func_evals;
        H->iters = iters;
        H->evals = evals;
        H->stop = stop;
        H->hist_len = hist_len;
        H->head = head;
        H->loss = loss;
        H->prev_loss = loss;
        H->H_diag = H_diag;
        H->t = t;
    }
}

// ---- the one-thread kernels of both engines (lbfgs_common.h) ---------------------
__global__ void lbfgs_init_kernel(HeaderBase *H, int64_t n, int64_t m, int64_t ld,
                                  int64_t *extra_word, int64_t extra) {
    H->n = n;
    H->history_size = m;
    H->ld = ld;
    H->H_diag = 1.0f;
    if (extra_word) *extra_word = extra;
}

__global__ void lbfgs_begin_kernel(HeaderBase *H) {
    H->iters = 0;
    H->evals = 0;
    H->stop = 0;
}

// a fused run's per-step snapshot: the six status words
__global__ void lbfgs_snapshot_kernel(const HeaderBase *H, int64_t *out) {
    out[0] = H->n_iter;
    out[1] = H->func_evals;
    out[2] = H->iters;
    out[3] = H->evals;
    out[4] = H->stop;
    out[5] = H->hist_len;
}

template <int NV>
void launch_iterate(char *state, const Table &T, const float *loss, float lr, int max_iter,
                    int max_eval, double tg, double tc, hipStream_t s) {
    hipLaunchKernelGGL(lbfgs_iterate_kernel<NV>, dim3(1), dim3(kThreads), 0, s, state, T, loss, lr,
                       max_iter, max_eval, tg, tc);
}

// the iterate launch for n parameters: the size class by 16-B chunks per thread
hipError_t enqueue_iterate(char *st, const Table &T, int64_t n, const float *loss, float lrf,
                           int max_iter, int max_eval, double tol_grad, double tol_change,
                           hipStream_t s) {
    const int64_t chunks = row_ld(n) / 4;
    if (chunks <= 1 * kThreads)
        launch_iterate<1>(st, T, loss, lrf, max_iter, max_eval, tol_grad, tol_change, s);
    else if (chunks <= 2 * kThreads)
        launch_iterate<2>(st, T, loss, lrf, max_iter, max_eval, tol_grad, tol_change, s);
    else if (chunks <= 4 * kThreads)
        launch_iterate<4>(st, T, loss, lrf, max_iter, max_eval, tol_grad, tol_change, s);
    else if (chunks <= 8 * kThreads)
        launch_iterate<8>(st, T, loss, lrf, max_iter, max_eval, tol_grad, tol_change, s);
    else
        launch_iterate<16>(st, T, loss, lrf, max_iter, max_eval, tol_grad, tol_change, s);
    return hipGetLastError();
}

}  // namespace

int state_init(const char *what, const Engine &E, void *state, int64_t bytes, int64_t need,
               int64_t n, int32_t history_size, int64_t *extra_word, int64_t extra,
               hipStream_t s) {
    SGC_REQUIRE(bytes >= need, SGC_ENOMEM, "%s: state %lld < %lld bytes", what, (long long)bytes,
                (long long)need);
    SGC_REQUIRE(reinterpret_cast<uintptr_t>(state) % 256 == 0, SGC_EINVAL,
                "%s: state not 256-B aligned", what);
    SGC_HIP_CHECK(hipMemsetAsync(state, 0, (size_t)need, s));
    hipLaunchKernelGGL(lbfgs_init_kernel, dim3(1), dim3(1), 0, s,
                       reinterpret_cast<HeaderBase *>(state), n, (int64_t)history_size, row_ld(n),
                       extra_word, extra);
    SGC_HIP_CHECK(hipGetLastError());
    record_state(state, n, history_size, E);
    return SGC_OK;
}

int state_snapshot(const void *state, int64_t *out, hipStream_t s) {
    hipLaunchKernelGGL(lbfgs_snapshot_kernel, dim3(1), dim3(1), 0, s,
                       reinterpret_cast<const HeaderBase *>(state), out);
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

int lbfgs_begin_step(const char *what, void *state, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "%s: null state", what);
    hipLaunchKernelGGL(lbfgs_begin_kernel, dim3(1), dim3(1), 0, s,
                       reinterpret_cast<HeaderBase *>(state));
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

int lbfgs_read_status(const char *what, const void *state, int64_t *out_host, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "%s: null state", what);
    SGC_REQUIRE(out_host, SGC_EINVAL, "%s: null out_host", what);
    SGC_HIP_CHECK(hipMemcpyAsync(out_host, state, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SGC_HIP_CHECK(hipStreamSynchronize(s));
    return SGC_OK;
}

// ---- the narrow engine's entries ---------------------------------------------------
int64_t lbfgs_workspace(int64_t n, int32_t history_size) {
    if (check_shape("lbfgs_workspace", n, history_size, kE)) return 0;
    return state_bytes(n, history_size);
}

int lbfgs_init(void *state, int64_t bytes, int64_t n, int32_t history_size, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_init: null state");
    if (const int rc = check_shape("lbfgs_init", n, history_size, kE)) return rc;
    return state_init("lbfgs_init", kE, state, bytes, state_bytes(n, history_size), n,
                      history_size, nullptr, 0, s);
}

int lbfgs_iterate(void *state, int32_t n_tensors, float *const *params, const float *const *grads,
                  const int64_t *numels, const float *loss, double lr, int32_t max_iter,
                  int32_t max_eval, double tol_grad, double tol_change, hipStream_t s) {
    return iterate_entry<int32_t>("lbfgs_iterate", kE, enqueue_iterate, state, n_tensors, params,
                                  grads, numels, loss, lr, max_iter, max_eval, tol_grad,
                                  tol_change, s);
}

// ---- sgc_train_lbfgs_f32: run_train_steps (lbfgs_common.h) on the four launches
// of sgc_linear_xent_f32 behind the stop word (xent.hip) ---------------------------
int64_t train_lbfgs_workspace(int64_t M, int64_t K, int64_t C) {
    if (M <= 0 || K <= 0 || C <= 0 || C > 64 || C * K > kMaxN) return 0;
    return train_workspace_bytes(K, C, xent_workspace_bytes(M, K, C));
}

int train_lbfgs(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels, int64_t M,
                int64_t K, int64_t C, void *state, int32_t steps, double lr, int32_t max_iter,
                int32_t max_eval, double tol_grad, double tol_change, float *loss_trace,
                int64_t *status_trace, void *ws, int64_t ws_bytes, hipStream_t s) {
    SGC_REQUIRE(steps >= 0, SGC_EINVAL, "train_lbfgs: steps=%d < 0", steps);
    SGC_REQUIRE(M > 0 && K > 0 && C > 0 && C <= 64 && ldx >= K, SGC_EINVAL,
                "train_lbfgs: bad shape M=%lld K=%lld C=%lld ldx=%lld (1 <= C <= 64, ldx >= K)",
                (long long)M, (long long)K, (long long)C, (long long)ldx);
    SGC_REQUIRE(max_iter >= 1, SGC_EINVAL, "train_lbfgs: max_iter=%d < 1", max_iter);
    SGC_REQUIRE(X && W && labels && state && ws, SGC_EINVAL, "train_lbfgs: null pointer");
    SGC_REQUIRE(reinterpret_cast<uintptr_t>(X) % 4 == 0, SGC_EINVAL,
                "train_lbfgs: X not 4-B aligned");
    const int64_t ck = C * K, n = ck + (b ? C : 0);
    SGC_REQUIRE(n <= kMaxN, SGC_ERANGE, "train_lbfgs: n=%lld > %lld parameters", (long long)n,
                (long long)kMaxN);
    if (const int rc = xent_closure_check("train_lbfgs", M, K, C, ldx)) return rc;
    const int64_t need = train_lbfgs_workspace(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "train_lbfgs: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    if (steps == 0) return SGC_OK;
    auto closure = [&](const StateShape &, const int64_t *stop, float *loss, float *dW, float *db,
                       void *xent_ws) {
        return xent_closure(stop, X, ldx, W, b, labels, M, K, C, loss, dW, db, xent_ws, s);
    };
    return run_train_steps<int32_t>("train_lbfgs", kE, closure, enqueue_iterate, W, b, K, C, state,
                                    steps, lr, max_iter, max_eval, tol_grad, tol_change,
                                    loss_trace, status_trace, ws, s);
}

// ---- sgc_train_lbfgs_x16: the same loop, the closure on 16-bit X ---------------
// (xent16.hip: launches A, B and C of sgc_linear_xent_x16 behind the stop word)
int64_t train_lbfgs_x16_workspace(int64_t M, int64_t K, int64_t C) {
    const int64_t xw = linear_xent_x16_workspace_bytes(M, K, C);
    if (xw == 0 || C * K + C > kMaxN) return 0;
    return train_workspace_bytes(K, C, xw);
}

int train_lbfgs_x16(const void *X, int32_t x_dtype, int64_t ldx, float *W, float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, void *state,
                    int32_t steps, double lr, int32_t max_iter, int32_t max_eval, double tol_grad,
                    double tol_change, float *loss_trace, int64_t *status_trace, void *ws,
                    int64_t ws_bytes, hipStream_t s) {
    SGC_REQUIRE(steps >= 0, SGC_EINVAL, "train_lbfgs_x16: steps=%d < 0", steps);
    if (const int rc = xent_x16_closure_check("train_lbfgs_x16", X, x_dtype, ldx, M, K, C))
        return rc;
    SGC_REQUIRE(max_iter >= 1, SGC_EINVAL, "train_lbfgs_x16: max_iter=%d < 1", max_iter);
    SGC_REQUIRE(X && W && labels && state && ws, SGC_EINVAL, "train_lbfgs_x16: null pointer");
    const int64_t n = C * K + (b ? C : 0);
    SGC_REQUIRE(C * K + C <= kMaxN, SGC_ERANGE, "train_lbfgs_x16: n=%lld > %lld parameters",
                (long long)n, (long long)kMaxN);
    const int64_t need = train_lbfgs_x16_workspace(M, K, C);
    SGC_REQUIRE(ws_bytes >= need, SGC_ENOMEM, "train_lbfgs_x16: workspace %lld < %lld",
                (long long)ws_bytes, (long long)need);
    if (steps == 0) return SGC_OK;
    auto closure = [&](const StateShape &, const int64_t *stop, float *loss, float *dW, float *db,
                       void *xent_ws) {
        return xent_x16_closure(stop, X, x_dtype, ldx, W, b, labels, M, K, C, loss, dW, db, xent_ws,
                                s);
    };
    return run_train_steps<int32_t>("train_lbfgs_x16", kE, closure, enqueue_iterate, W, b, K, C,
                                    state, steps, lr, max_iter, max_eval, tol_grad, tol_change,
                                    loss_trace, status_trace, ws, s);
}

SGC_WARM_UNIT(warm_lbfgs)

}  // namespace sgc
