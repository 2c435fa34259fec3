// lbfgs_common.h -- what the two L-BFGS engines share: lbfgs.hip (one workgroup,
// the vector in registers, n <= 65,536) and lbfgs_wide.hip (Gram form over the
// whole machine).  One definition each of the state header, the tensor table,
// torch's decision logic, the state registry and the fused training loop; the
// engines differ in the arithmetic between the decisions only.
//
// Everything here is a template, `inline` or `constexpr`, so both units may
// include it; the three one-thread kernels and the host calls that launch them
// are defined once, in lbfgs.hip, and declared at the end of this file.
#pragma once

#include <cstddef>
#include <map>
#include <mutex>

#include "common.h"
#include "internal.h"

namespace sgc {

constexpr int kMaxTensors = 16;
constexpr int kMaxHistory = 1024;  // per-pair scalars of the ring live in LDS during a launch
constexpr int64_t kHeaderBytes = 256;

// The scalar block at the start of either state; the first six words are what
// sgc_lbfgs_read_status copies back (include/sgc_amd.h documents them).  The
// wide state's header goes on behind it.
struct HeaderBase {
    int64_t n_iter, func_evals, iters, evals, stop, hist_len;
    int64_t head;  // ring slot of the oldest pair
    int64_t n, history_size, ld;
    double loss, prev_loss;
    float H_diag, t;
};
static_assert(sizeof(HeaderBase) == 104, "documented header prefix");
static_assert(offsetof(HeaderBase, n_iter) == 0 && offsetof(HeaderBase, hist_len) == 40,
              "the six status words come first");

typedef float f4 __attribute__((ext_vector_type(4)));

// Parameters and gradients as separate tensors at arbitrary offsets of the
// flat vector.  Off: int32_t in the narrow kernel (its register budget),
// int64_t in the wide ones.
template <typename Off> struct Tensors {
    float *p[kMaxTensors];
    const float *g[kMaxTensors];
    Off off[kMaxTensors + 1];  // prefix sums of the numels
    int32_t count;
};


__host__ __device__ constexpr int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
__host__ __device__ constexpr int64_t row_ld(int64_t n) { return round_up(n, 32); }
__host__ __device__ constexpr int64_t scalars_bytes(int64_t m) { return round_up(m * 4, 256); }

// max that keeps a NaN (torch's abs().max() does): fmax would drop it
__device__ __forceinline__ double nan_max(double a, double b) {
    return a != a ? a : (b != b ? b : (a > b ? a : b));
}

template <typename Off>
__device__ __forceinline__ f4 load_chunk(const float *row, Off nc, Off c) {
    return c < nc ? reinterpret_cast<const f4 *>(row)[c] : f4{0.f, 0.f, 0.f, 0.f};
}

// element j of the flat gradient (NULL tensor: zeros, as torch substitutes)
template <typename Off>
__device__ __forceinline__ float flat_grad(const Tensors<Off> &T, Off j) {
    float v = 0.0f;
    for (int ti = 0; ti < T.count; ++ti)
        if (j >= T.off[ti] && j < T.off[ti + 1]) {
            const float *gp = T.g[ti];
            if (gp) v = gp[j - T.off[ti]];
        }
    return v;
}

// x_j += t d[e], a single fmaf, in whichever tensor holds element j
template <typename Off>
__device__ __forceinline__ void update_param(const Tensors<Off> &T, Off j, float t, const f4 &d,
                                             int e) {
    for (int ti = 0; ti < T.count; ++ti)
        if (j >= T.off[ti] && j < T.off[ti + 1]) {
            float *pp = T.p[ti] + (j - T.off[ti]);
            *pp = fmaf(t, d[e], *pp);
        }
}

// ---- torch's decisions, over plain scalars ---------------------------------------
// Comparisons are written so that a NaN takes torch's branch: all of torch's
// tests are false on NaN, so a NaN loss or gradient stops nothing and pushes
// no history pair.

// The termination tests of the iteration just taken, after closure number
// `evals` of the step (already counted): the stop code, 0 to go on.
__device__ __forceinline__ int entry_stop(int evals, int max_eval, double gmax, double tdmax,
                                          double loss, double prev_loss, double tol_grad,
                                          double tol_change) {
    int stop = 0;
    if (evals == 1) {  // first closure of the step
        if (gmax <= tol_grad) stop = SGC_LBFGS_STOP_OPT_AT_ENTRY;
    } else {  // torch's tests after the re-evaluation, in its order
        if (evals >= max_eval) stop = SGC_LBFGS_STOP_MAX_EVAL;
        else if (gmax <= tol_grad) stop = SGC_LBFGS_STOP_OPT;
        else if (tdmax <= tol_change) stop = SGC_LBFGS_STOP_STEP_SMALL;
        else if (fabs(loss - prev_loss) < tol_change) stop = SGC_LBFGS_STOP_LOSS_CHANGE;
    }
    return stop;
}

// The memory update of an iteration that goes on: whether the pair (s, y) is
// accepted (never in the first iteration, `first`, whose s and y are zero),
// the ring slot it takes (the oldest pair's when the ring is full: `evict`),
// the new head / hist_len and H_diag.  on_push(slot) runs where the pair is
// accepted (the narrow kernel stores ro there).
struct PairDecision {
    bool push, evict;
    int slot, head, hist_len;
    float H_diag;
};
template <typename OnPush>
__device__ __forceinline__ PairDecision accept_pair(bool first, float ys, float yy, int m, int head,
                                                    int hist_len, float H_diag, OnPush on_push) {
    PairDecision D;
    D.push = !first && (double)ys > 1e-10;
    D.evict = D.push && hist_len == m;
    D.slot = 0;
    if (D.push) {
        if (D.evict) {  // drop the oldest pair
            D.slot = head;
            head = (head + 1) % m;
        } else {
            D.slot = (head + hist_len) % m;
            hist_len += 1;
        }
        H_diag = ys / yy;
        on_push(D.slot);
    }
    if (first) H_diag = 1.0f;
    D.head = head;
    D.hist_len = hist_len;
    D.H_diag = H_diag;
    return D;
}

// the step size of the new direction: min(1, 1 / |g|_1) lr in the first iteration
__device__ __forceinline__ float step_size(bool first, float g1, float lr) {
    return first ? ((1.0f / g1 < 1.0f) ? 1.0f / g1 : 1.0f) * lr : lr;
}

// ---- host side ---------------------------------------------------------------------
// What tells the two engines apart in an argument check.
struct Engine {
    bool wide;
    int64_t max_n;
    const char *limit;  // how an n past max_n is worded
    const char *init;   // the call that builds this engine's state
};
constexpr Engine kNarrowEngine{false, 65536, "> 65536", "sgc_lbfgs_init"};
constexpr Engine kWideEngine{true, INT32_MAX - 1, ">= 2^31 - 1", "sgc_lbfgs_wide_init"};

// What either init recorded of each state, for the argument checks of the
// later calls (the state itself is device memory the host never reads).  One
// map for both engines: an entry lives until either init is called on the same
// address again, which replaces it, so a caller that frees a state and reuses
// the address must initialise it anew, and a call of the other engine on it is
// refused.
struct StateShape {
    int64_t n, m;
    bool wide;
};
inline std::mutex g_states_mu;
inline std::map<const void *, StateShape> g_states;

inline void record_state(const void *state, int64_t n, int64_t m, const Engine &E) {
    std::lock_guard<std::mutex> lock(g_states_mu);
    g_states[state] = StateShape{n, m, E.wide};
}

inline int find_state(const char *what, const void *state, const Engine &E, StateShape &out) {
    std::lock_guard<std::mutex> lock(g_states_mu);
    auto it = g_states.find(state);
    SGC_REQUIRE(it != g_states.end() && it->second.wide == E.wide, SGC_EINVAL,
                "%s: state not initialised by %s", what, E.init);
    out = it->second;
    return SGC_OK;
}

inline int check_shape(const char *what, int64_t n, int64_t history_size, const Engine &E) {
    SGC_REQUIRE(n >= 1, SGC_EINVAL, "%s: n=%lld < 1", what, (long long)n);
    SGC_REQUIRE(n <= E.max_n, SGC_ERANGE, "%s: n=%lld %s parameters", what, (long long)n, E.limit);
    SGC_REQUIRE(history_size >= 1, SGC_EINVAL, "%s: history_size=%lld < 1", what,
                (long long)history_size);
    SGC_REQUIRE(history_size <= kMaxHistory, SGC_ERANGE, "%s: history_size=%lld > %d", what,
                (long long)history_size, kMaxHistory);
    return SGC_OK;
}

// The kernels' tensor table from the caller's host tables of 1..16 tensors; n:
// the numels' sum.  (A NULL parameter is the caller's to refuse: after the
// state's checks.)
template <typename Off>
int build_table(const char *what, const Engine &E, int32_t n_tensors, float *const *params,
                const float *const *grads, const int64_t *numels, Tensors<Off> &T, int64_t &n) {
    n = 0;
    for (int i = 0; i < n_tensors; ++i) {
        SGC_REQUIRE(numels[i] >= 0, SGC_EINVAL, "%s: numels[%d]=%lld < 0", what, i,
                    (long long)numels[i]);
        T.off[i] = (Off)n;
        n += numels[i];
        SGC_REQUIRE(n <= E.max_n, SGC_ERANGE, "%s: n %s parameters", what, E.limit);
    }
    SGC_REQUIRE(n >= 1, SGC_EINVAL, "%s: n=0 < 1", what);
    for (int i = 0; i < kMaxTensors; ++i) {
        T.p[i] = i < n_tensors ? params[i] : nullptr;
        T.g[i] = i < n_tensors ? grads[i] : nullptr;
    }
    for (int i = n_tensors; i <= kMaxTensors; ++i) T.off[i] = (Off)n;
    T.count = n_tensors;
    return SGC_OK;
}

// sgc_lbfgs_iterate_f32 / sgc_lbfgs_wide_iterate_f32: the argument checks, then
// enqueue(state, T, n, loss, lr, max_iter, max_eval, tol_grad, tol_change, s),
// the engine's launches of one iteration.
template <typename Off, typename Enqueue>
int iterate_entry(const char *what, const Engine &E, Enqueue &&enqueue, void *state,
                  int32_t n_tensors, float *const *params, const float *const *grads,
                  const int64_t *numels, const float *loss, double lr, int32_t max_iter,
                  int32_t max_eval, double tol_grad, double tol_change, hipStream_t s) {
    SGC_REQUIRE(state, SGC_EINVAL, "%s: null state", what);
    SGC_REQUIRE(n_tensors >= 1 && n_tensors <= kMaxTensors, SGC_EINVAL,
                "%s: n_tensors=%d outside 1..%d", what, n_tensors, kMaxTensors);
    SGC_REQUIRE(params && grads && numels, SGC_EINVAL, "%s: null pointer table", what);
    SGC_REQUIRE(max_iter >= 1, SGC_EINVAL, "%s: max_iter=%d < 1", what, max_iter);
    Tensors<Off> T;
    int64_t n;
    if (const int rc = build_table(what, E, n_tensors, params, grads, numels, T, n)) return rc;
    StateShape sh;
    if (const int rc = find_state(what, state, E, sh)) return rc;
    SGC_REQUIRE(sh.n == n, SGC_EINVAL,
                "%s: numels sum to %lld, the state was initialised for n=%lld", what, (long long)n,
                (long long)sh.n);
    for (int i = 0; i < n_tensors; ++i)
        SGC_REQUIRE(params[i] || numels[i] == 0, SGC_EINVAL, "%s: null parameter %d", what, i);
    SGC_REQUIRE(loss, SGC_EINVAL, "%s: null loss", what);
    const hipError_t e = enqueue(reinterpret_cast<char *>(state), T, n, loss, (float)lr, max_iter,
                                 max_eval, tol_grad, tol_change, s);
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return SGC_OK;
}

// Defined in lbfgs.hip (with their one-thread kernels), for both engines.
// state_init: zero `need` bytes, write n, history_size, ld and H_diag = 1 into
// the header and `extra` into *extra_word (the wide header's tile count; NULL:
// none), record the state in the registry.
int state_init(const char *what, const Engine &E, void *state, int64_t bytes, int64_t need,
               int64_t n, int32_t history_size, int64_t *extra_word, int64_t extra, hipStream_t s);
// state_snapshot: the six status words into out, on the device
int state_snapshot(const void *state, int64_t *out, hipStream_t s);

// workspace of a fused training call: gradient [C*K + C] | loss | the closure's
// workspace of closure_bytes, each 256-B aligned
constexpr int64_t train_workspace_bytes(int64_t K, int64_t C, int64_t closure_bytes) {
    return 256 + round_up((C * K + C) * 4, 256) + 256 + closure_bytes;
}

// ---- `steps` whole steps enqueued by one host call --------------------------------
// The loop of reddit.py:51-64 for the SGC classifier with the closure on the
// device side too: per step the reset of lbfgs_begin_step, then max_iter times
// [closure, iterate], then the status snapshot.  closure(sh, stop, loss, dW, db,
// closure_ws) enqueues one closure behind the stop word: it writes loss, dW
// and db into the workspace (the flat gradient, W then b), which the iterate
// launches read as their two gradient tensors.  Once an iteration has set the
// stop word, the rest of the step's launches return at entry: nothing moves
// until the next step's reset.  The first closure of step s runs always (the
// reset precedes it) and writes its loss straight into loss_trace[s].
// Arguments are checked by the caller; enqueue as for iterate_entry.
template <typename Off, typename Closure, typename Enqueue>
int run_train_steps(const char *what, const Engine &E, Closure &&closure, Enqueue &&enqueue,
                    float *W, float *b, int64_t K, int64_t C, void *state, int32_t steps, double lr,
                    int32_t max_iter, int32_t max_eval, double tol_grad, double tol_change,
                    float *loss_trace, int64_t *status_trace, void *ws, hipStream_t s) {
    const int64_t ck = C * K;
    char *p = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
    float *grad = reinterpret_cast<float *>(p);
    p += round_up((ck + C) * 4, 256);
    float *loss_slot = reinterpret_cast<float *>(p);
    p += 256;
    void *closure_ws = p;
    // (the table the stepwise entry builds for [W, b]: the same kernel arguments)
    float *const params[2] = {W, b};
    const float *const grads[2] = {grad, grad + ck};
    const int64_t numels[2] = {ck, C};
    Tensors<Off> T;
    int64_t n;
    if (const int rc = build_table(what, E, b ? 2 : 1, params, grads, numels, T, n)) return rc;
    StateShape sh;
    if (const int rc = find_state(what, state, E, sh)) return rc;
    SGC_REQUIRE(sh.n == n, SGC_EINVAL,
                "%s: C*K%s = %lld parameters, the state was initialised for n=%lld", what,
                b ? " + C" : "", (long long)n, (long long)sh.n);
    char *st = reinterpret_cast<char *>(state);
    const int64_t *stop = &reinterpret_cast<HeaderBase *>(state)->stop;  // (never read here)
    for (int32_t step = 0; step < steps; ++step) {
        if (const int rc = lbfgs_begin_step(what, state, s)) return rc;
        for (int32_t it = 0; it < max_iter; ++it) {
            float *loss = (it == 0 && loss_trace) ? loss_trace + step : loss_slot;
            if (const int rc = closure(sh, stop, loss, grad, b ? grad + ck : nullptr, closure_ws))
                return rc;
            const hipError_t e =
                enqueue(st, T, n, loss, (float)lr, max_iter, max_eval, tol_grad, tol_change, s);
            SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "%s launch failed: %s", what,
                        hipGetErrorString(e));
        }
        if (status_trace)
            if (const int rc = state_snapshot(state, status_trace + 6 * (int64_t)step, s))
                return rc;
    }
    return SGC_OK;
}

}  // namespace sgc
