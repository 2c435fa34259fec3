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
// Comparisons are written so that a NaN takes torch's branch: all of torch's
// tests are false on NaN, so a NaN loss or gradient stops nothing and pushes
// no history pair.
#include <cmath>
#include <map>
#include <mutex>

#include "common.h"
#include "internal.h"

namespace sgc {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxTensors = 16;
constexpr int kMaxHistory = 1024;  // ro / al of the ring live in LDS during a launch
constexpr int64_t kMaxN = 65536;   // 64 register elements per thread
constexpr int64_t kHeaderBytes = 256;

// The scalar block at the start of the state; the first six words are what
// sgc_lbfgs_read_status copies back (include/sgc_amd.h documents them).
struct Header {
    int64_t n_iter, func_evals, iters, evals, stop, hist_len;
    int64_t head;  // ring slot of the oldest pair
    int64_t n, history_size, ld;
    double loss, prev_loss;
    float H_diag, t;
};
static_assert(sizeof(Header) <= kHeaderBytes, "header block");

struct Tensors {
    float *p[kMaxTensors];
    const float *g[kMaxTensors];
    int32_t off[kMaxTensors + 1];  // prefix sums of the numels
    int32_t count;
};

typedef float f4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
__host__ __device__ constexpr int64_t row_ld(int64_t n) { return round_up(n, 32); }
__host__ __device__ constexpr int64_t scalars_bytes(int64_t m) { return round_up(m * 4, 256); }

// state: header | ro[m] | d[ld] | prev_g[ld] | S[m][ld] | Y[m][ld]
int64_t state_bytes(int64_t n, int64_t m) {
    return kHeaderBytes + scalars_bytes(m) + (2 + 2 * m) * row_ld(n) * 4;
}

// max that keeps a NaN (torch's abs().max() does): fmax would drop it
__device__ __forceinline__ double nan_max(double a, double b) {
    return a != a ? a : (b != b ? b : (a > b ? a : b));
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

__device__ __forceinline__ f4 load_chunk(const float *row, int nc, int c) {
    return c < nc ? reinterpret_cast<const f4 *>(row)[c] : f4{0.f, 0.f, 0.f, 0.f};
}

template <int NV>
__device__ __forceinline__ void load_row(const float *row, int nc, f4 (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = load_chunk(row, nc, threadIdx.x + kThreads * k);
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
    for (int k = 0; k < NV; ++k) dot_chunk(acc, load_chunk(row, nc, threadIdx.x + kThreads * k), q[k]);
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
        const f4 a = load_chunk(row, nc, threadIdx.x + kThreads * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[k][e] = fmaf(coef, a[e], q[k][e]);
    }
}

// element j of the flat gradient (NULL tensor: zeros, as torch substitutes)
__device__ __forceinline__ float flat_grad(const Tensors &T, int j) {
    float v = 0.0f;
    for (int ti = 0; ti < T.count; ++ti)
        if (j >= T.off[ti] && j < T.off[ti + 1]) {
            const float *gp = T.g[ti];
            if (gp) v = gp[j - T.off[ti]];
        }
    return v;
}

// NV 16-B chunks per thread.  What stays in registers across a reduction's
// barrier besides q: the next S row and the Y row of the pair up to NV = 4
// (their loads do not wait for the reduction), nothing above it, where the
// rows are streamed through (q alone is 32 / 64 registers of the 128 a wave
// of a 1024-thread workgroup has).
template <int NV>
__global__ __launch_bounds__(kThreads) void lbfgs_iterate_kernel(
    char *state, Tensors T, const float *__restrict__ loss_ptr, float lr, int max_iter,
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
            const f4 pg = load_chunk(pg_g, nc, c), d = load_chunk(d_g, nc, c);
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
        if (evals == 1) {  // first closure of the step
            if (gmax <= tol_grad) stop = SGC_LBFGS_STOP_OPT_AT_ENTRY;
        } else {  // torch's tests after the re-evaluation, in its order
            if (evals >= max_eval) stop = SGC_LBFGS_STOP_MAX_EVAL;
            else if (gmax <= tol_grad) stop = SGC_LBFGS_STOP_OPT;
            else if (r[2] <= tol_change) stop = SGC_LBFGS_STOP_STEP_SMALL;
            else if (fabs(loss - H->prev_loss) < tol_change) stop = SGC_LBFGS_STOP_LOSS_CHANGE;
        }
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
        const bool push = !first && (double)ys > 1e-10;
        int slot = 0;
        if (push) {
            if (hist_len == m) {  // drop the oldest pair
                slot = head;
                head = (head + 1) % m;
            } else {
                slot = (head + hist_len) % m;
                hist_len += 1;
            }
            H_diag = ys / yy;
            if (tid == 0) ro_g[slot] = ro_s[slot] = 1.0f / ys;
        }
        if (first) H_diag = 1.0f;
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
        t = first ? ((1.0f / g1 < 1.0f) ? 1.0f / g1 : 1.0f) * lr : lr;
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
                    for (int ti = 0; ti < T.count; ++ti)
                        if (j >= T.off[ti] && j < T.off[ti + 1]) {
                            float *pp = T.p[ti] + (j - T.off[ti]);
                            *pp = fmaf(t, q[k][e], *pp);
                        }
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

__global__ void lbfgs_init_kernel(Header *H, int64_t n, int64_t m, int64_t ld) {
    H->n = n;
    H->history_size = m;
    H->ld = ld;
    H->H_diag = 1.0f;
}

__global__ void lbfgs_begin_kernel(Header *H) {
    H->iters = 0;
    H->evals = 0;
    H->stop = 0;
}

// What sgc_lbfgs_init recorded of each state, for the argument checks of the
// later calls (the state itself is device memory the host never reads).
struct Shape {
    int64_t n, m;
};
std::mutex g_states_mu;
std::map<const void *, Shape> g_states;

template <int NV>
void launch_iterate(char *state, const Tensors &T, const float *loss, float lr, int max_iter,
                    int max_eval, double tg, double tc, hipStream_t s) {
    hipLaunchKernelGGL(lbfgs_iterate_kernel<NV>, dim3(1), dim3(kThreads), 0, s, state, T, loss, lr,
                       max_iter, max_eval, tg, tc);
}

// the iterate launch for n parameters: the size class by 16-B chunks per thread
hipError_t enqueue_iterate(char *st, const Tensors &T, int64_t n, const float *loss, float lrf,
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

// sgc_train_lbfgs_f32's per-step snapshot: the six status words, one thread
__global__ void lbfgs_snapshot_kernel(const Header *H, int64_t *out) {
    out[0] = H->n_iter;
    out[1] = H->func_evals;
    out[2] = H->iters;
    out[3] = H->evals;
    out[4] = H->stop;
    out[5] = H->hist_len;
}

}  // namespace

static int check_shape(const char *what, int64_t n, int64_t history_size);

int64_t lbfgs_workspace(int64_t n, int32_t history_size) {
    if (check_shape("lbfgs_workspace", n, history_size)) return 0;
    return state_bytes(n, history_size);
}

static int check_shape(const char *what, int64_t n, int64_t history_size) {
    SGC_REQUIRE(n >= 1, SGC_EINVAL, "%s: n=%lld < 1", what, (long long)n);
    SGC_REQUIRE(n <= kMaxN, SGC_ERANGE, "%s: n=%lld > %lld parameters", what, (long long)n,
                (long long)kMaxN);
    SGC_REQUIRE(history_size >= 1, SGC_EINVAL, "%s: history_size=%lld < 1", what,
                (long long)history_size);
    SGC_REQUIRE(history_size <= kMaxHistory, SGC_ERANGE, "%s: history_size=%lld > %d", what,
                (long long)history_size, kMaxHistory);
    return SGC_OK;
}

int lbfgs_init(void *state, int64_t bytes, int64_t n, int32_t history_size, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_init: null state");
    if (const int rc = check_shape("lbfgs_init", n, history_size)) return rc;
    SGC_REQUIRE(bytes >= state_bytes(n, history_size), SGC_ENOMEM,
                "lbfgs_init: state %lld < %lld bytes", (long long)bytes,
                (long long)state_bytes(n, history_size));
    SGC_REQUIRE(reinterpret_cast<uintptr_t>(state) % 256 == 0, SGC_EINVAL,
                "lbfgs_init: state not 256-B aligned");
    SGC_HIP_CHECK(hipMemsetAsync(state, 0, (size_t)state_bytes(n, history_size), s));
    hipLaunchKernelGGL(lbfgs_init_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<Header *>(state),
                       n, (int64_t)history_size, row_ld(n));
    SGC_HIP_CHECK(hipGetLastError());
    std::lock_guard<std::mutex> lock(g_states_mu);
    g_states[state] = Shape{n, history_size};
    return SGC_OK;
}

int lbfgs_begin_step(void *state, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_begin_step: null state");
    hipLaunchKernelGGL(lbfgs_begin_kernel, dim3(1), dim3(1), 0, s,
                       reinterpret_cast<Header *>(state));
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

int lbfgs_iterate(void *state, int32_t n_tensors, float *const *params, const float *const *grads,
                  const int64_t *numels, const float *loss, double lr, int32_t max_iter,
                  int32_t max_eval, double tol_grad, double tol_change, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_iterate: null state");
    SGC_REQUIRE(n_tensors >= 1 && n_tensors <= kMaxTensors, SGC_EINVAL,
                "lbfgs_iterate: n_tensors=%d outside 1..%d", n_tensors, kMaxTensors);
    SGC_REQUIRE(params && grads && numels, SGC_EINVAL, "lbfgs_iterate: null pointer table");
    SGC_REQUIRE(max_iter >= 1, SGC_EINVAL, "lbfgs_iterate: max_iter=%d < 1", max_iter);
    Tensors T;
    int64_t n = 0;
    for (int i = 0; i < kMaxTensors; ++i) {
        T.p[i] = nullptr;
        T.g[i] = nullptr;
    }
    for (int i = 0; i < n_tensors; ++i) {
        SGC_REQUIRE(numels[i] >= 0, SGC_EINVAL, "lbfgs_iterate: numels[%d]=%lld < 0", i,
                    (long long)numels[i]);
        T.off[i] = (int32_t)n;
        n += numels[i];
        SGC_REQUIRE(n <= kMaxN, SGC_ERANGE, "lbfgs_iterate: n > %lld parameters",
                    (long long)kMaxN);
    }
    SGC_REQUIRE(n >= 1, SGC_EINVAL, "lbfgs_iterate: n=0 < 1");
    for (int i = n_tensors; i <= kMaxTensors; ++i) T.off[i] = (int32_t)n;
    T.count = n_tensors;
    {
        std::lock_guard<std::mutex> lock(g_states_mu);
        auto it = g_states.find(state);
        SGC_REQUIRE(it != g_states.end(), SGC_EINVAL,
                    "lbfgs_iterate: state not initialised by sgc_lbfgs_init");
        SGC_REQUIRE(it->second.n == n, SGC_EINVAL,
                    "lbfgs_iterate: numels sum to %lld, the state was initialised for n=%lld",
                    (long long)n, (long long)it->second.n);
    }
    for (int i = 0; i < n_tensors; ++i) {
        SGC_REQUIRE(params[i] || numels[i] == 0, SGC_EINVAL, "lbfgs_iterate: null parameter %d", i);
        T.p[i] = params[i];
        T.g[i] = grads[i];
    }
    SGC_REQUIRE(loss, SGC_EINVAL, "lbfgs_iterate: null loss");
    const hipError_t e = enqueue_iterate(reinterpret_cast<char *>(state), T, n, loss, (float)lr,
                                         max_iter, max_eval, tol_grad, tol_change, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "lbfgs_iterate launch failed: %s", hipGetErrorString(e));
    return SGC_OK;
}

int lbfgs_read_status(const void *state, int64_t *out_host, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "lbfgs_read_status: null state");
    SGC_REQUIRE(out_host, SGC_EINVAL, "lbfgs_read_status: null out_host");
    SGC_HIP_CHECK(hipMemcpyAsync(out_host, state, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SGC_HIP_CHECK(hipStreamSynchronize(s));
    return SGC_OK;
}

// ---- sgc_train_lbfgs_f32: `steps` whole steps enqueued by one host call ------
// The loop of reddit.py:51-64 for the SGC classifier with the closure on the
// device side too: per step the reset of lbfgs_begin_step, then max_iter times
// [the four launches of sgc_linear_xent_f32 behind the stop word (xent.hip),
// lbfgs_iterate_kernel], then the status snapshot.  The closure writes loss,
// dW and db into the workspace (the flat gradient, W then b), which the
// iterate launch reads as its two gradient tensors.  Once an iterate launch has
// set the stop word, the rest of the step's launches return at entry: nothing
// moves until the next step's reset.  The first closure of step s runs always
// (the reset precedes it) and writes its loss straight into loss_trace[s].

// workspace: gradient [n] | loss | the fused step's workspace, each 256-B aligned
int64_t train_lbfgs_workspace(int64_t M, int64_t K, int64_t C) {
    if (M <= 0 || K <= 0 || C <= 0 || C > 64 || C * K > kMaxN) return 0;
    return 256 + round_up((C * K + C) * 4, 256) + 256 + xent_workspace_bytes(M, K, C);
}

// The steps' launches, shared by the fp32 and the 16-bit entry (arguments
// checked by the caller): closure(stop, loss, dW, db, xent_ws) enqueues one
// closure behind the stop word.
template <typename Closure>
static int run_train_steps(const char *what, Closure &&closure, float *W, float *b, int64_t K,
                           int64_t C, void *state, int32_t steps, double lr, int32_t max_iter,
                           int32_t max_eval, double tol_grad, double tol_change, float *loss_trace,
                           int64_t *status_trace, void *ws, hipStream_t s) {
    const int64_t ck = C * K, n = ck + (b ? C : 0);
    {
        std::lock_guard<std::mutex> lock(g_states_mu);
        auto it = g_states.find(state);
        SGC_REQUIRE(it != g_states.end(), SGC_EINVAL, "%s: state not initialised by sgc_lbfgs_init",
                    what);
        SGC_REQUIRE(it->second.n == n, SGC_EINVAL,
                    "%s: C*K%s = %lld parameters, the state was initialised for n=%lld", what,
                    b ? " + C" : "", (long long)n, (long long)it->second.n);
    }
    char *p = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
    float *grad = reinterpret_cast<float *>(p);
    p += round_up((ck + C) * 4, 256);
    float *loss_slot = reinterpret_cast<float *>(p);
    p += 256;
    void *xent_ws = p;
    Tensors T;
    for (int i = 0; i < kMaxTensors; ++i) {
        T.p[i] = nullptr;
        T.g[i] = nullptr;
    }
    // (the table lbfgs_iterate builds for [W, b]: the same kernel arguments)
    T.count = b ? 2 : 1;
    T.p[0] = W;
    T.g[0] = grad;
    T.off[0] = 0;
    if (b) {
        T.p[1] = b;
        T.g[1] = grad + ck;
        T.off[1] = (int32_t)ck;
    }
    for (int i = T.count; i <= kMaxTensors; ++i) T.off[i] = (int32_t)n;
    char *st = reinterpret_cast<char *>(state);
    Header *H = reinterpret_cast<Header *>(state);
    const int64_t *stop = &H->stop;  // (a device address: never read here)
    const float lrf = (float)lr;
    for (int32_t step = 0; step < steps; ++step) {
        hipLaunchKernelGGL(lbfgs_begin_kernel, dim3(1), dim3(1), 0, s, H);
        SGC_HIP_CHECK(hipGetLastError());
        for (int32_t it = 0; it < max_iter; ++it) {
            float *loss = (it == 0 && loss_trace) ? loss_trace + step : loss_slot;
            if (const int rc = closure(stop, loss, grad, b ? grad + ck : nullptr, xent_ws))
                return rc;
            const hipError_t e = enqueue_iterate(st, T, n, loss, lrf, max_iter, max_eval, tol_grad,
                                                 tol_change, s);
            SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "%s launch failed: %s", what,
                        hipGetErrorString(e));
        }
        if (status_trace) {
            hipLaunchKernelGGL(lbfgs_snapshot_kernel, dim3(1), dim3(1), 0, s, H,
                               status_trace + 6 * (int64_t)step);
            SGC_HIP_CHECK(hipGetLastError());
        }
    }
    return SGC_OK;
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
    auto closure = [&](const int64_t *stop, float *loss, float *dW, float *db, void *xent_ws) {
        return xent_closure(stop, X, ldx, W, b, labels, M, K, C, loss, dW, db, xent_ws, s);
    };
    return run_train_steps("train_lbfgs", closure, W, b, K, C, state, steps, lr, max_iter, max_eval,
                           tol_grad, tol_change, loss_trace, status_trace, ws, s);
}

// ---- sgc_train_lbfgs_x16: the same loop, the closure on 16-bit X ---------------
// (xent16.hip: launches A, B and C of sgc_linear_xent_x16 behind the stop word)
int64_t train_lbfgs_x16_workspace(int64_t M, int64_t K, int64_t C) {
    const int64_t xw = linear_xent_x16_workspace_bytes(M, K, C);
    if (xw == 0 || C * K + C > kMaxN) return 0;
    return 256 + round_up((C * K + C) * 4, 256) + 256 + xw;
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
    auto closure = [&](const int64_t *stop, float *loss, float *dW, float *db, void *xent_ws) {
        return xent_x16_closure(stop, X, x_dtype, ldx, W, b, labels, M, K, C, loss, dW, db, xent_ws,
                                s);
    };
    return run_train_steps("train_lbfgs_x16", closure, W, b, K, C, state, steps, lr, max_iter,
                           max_eval, tol_grad, tol_change, loss_trace, status_trace, ws, s);
}

SGC_WARM_UNIT(warm_lbfgs)

}  // namespace sgc
