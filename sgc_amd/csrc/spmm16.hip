// spmm16.hip -- CSR SpMM  Y = S[rows] . X  with X (and Y) stored in 16 bits
// (bfloat16 / float16) for gfx950: 16 bits in memory, fp32 everywhere else.
//
// Numerical contract: every output element is the ONE sequential fp32 FMA
// chain of spmm.hip -- acc = +0.0f; acc = fmaf(val[k], float(X[col[k], f]),
// acc) over the row's nonzeros in CSR order -- where widening a 16-bit
// element is exact, and the chain's fp32 value is rounded to the output type
// once, at the store (round to nearest even: x16.h), or stored as it is when
// Y is fp32.  S stays fp32.  So a hop equals fp32_spmm(S, X.float()).to(T)
// bit for bit, and the plan (light / heavy / hub rows) is a schedule only.
//
// What a hop costs is the 128-B lines its gathers touch: a
// 602-element row in 128-B rows of 640 spans 10 lines in 16 bits, 19 in fp32.
//
// Mapping (one wavefront per work item, as spmm_csr_kernel):
//   * a lane's load holds V = 8 / 4 / 2 / 1 elements (16 / 8 / 4 / 2 bytes:
//     the widest the row stride, the base address and the readable columns
//     allow; see g_x16_vec for launches of several slices), so a wave covers
//     a 64V-element segment of one X row per load -- 512 elements, 1 KB, at
//     V = 8 -- and keeps V fp32 accumulators;
//   * feature slices of 64V elements are grid y (one pass over S each);
//   * light item = one row of one slice, in the plan's length order; heavy
//     item = one 64 * min(V, 4)-element sub-chunk of a row above the heavy
//     threshold, scheduled first; hub rows run on the LDS-staged hub kernel
//     (hub.h: its loaders gather 16-bit elements and widen them as they
//     stage, the fp32 LDS image and the chain wave are spmm_hub_kernel's);
//   * row_chunks_pipe's loop: (col, val) of 64 nonzeros per coalesced load,
//     broadcast with v_readlane so the X row base is wave-uniform, U nonzeros
//     per step and two steps in flight, loads unpredicated and clamped to the
//     row's last nonzero, 32-bit row offsets when X spans < 4 GiB.
// Lanes past F load a valid address (feature 0) and never store; a lane's
// vector reaches past F only into columns the caller declared readable /
// writable (SGC_SPMM_X_PADDED / SGC_SPMM_Y_PADDED: up to F rounded up to 8).
#include "common.h"
#include "hub.h"
#include "internal.h"
#include "spmm_schedule.h"
#include "x16.h"

#include <algorithm>

namespace sgc {

// Schedule knobs (sgc_set_tuning; results never depend on them).
// "x16_vec": the widest lane vector a launch may take, 8 / 4 / 2 / 1 elements
// (a 64V-element slice per pass over S).  0 = auto: 16-B lanes while the
// launch is one slice (F <= 512), 8-B lanes -- 256-element slices, the fp32
// kernels' 512 B of live X per row -- when it takes several passes.
// Measured, bf16, interleaved, bit-identical (profiles/x16/knobs.log), ms per
// hop at 8 / 4: Reddit shape (602: slices 512 + 90 vs 256 + 256 + 90) 3.19 /
// 2.91; RMAT shape (256: one slice either way) 20.03 / 20.78; Pubmed shape
// (500) 0.0418 / 0.0432.
int g_x16_vec = 0;
// "x16_step": nonzeros per step of a light row with 16-B lanes, 8 or 4 (two
// steps in flight: 8 holds 64 registers of gathered X per wave, 4 half of
// that and more waves per SIMD).  0 = auto: 4 on launches below kSmallRows16
// rows (latency-bound: Pubmed shape 0.0418 -> 0.0396 ms per hop), else 8
// (RMAT shape 20.03 vs 20.11 at 4; Reddit shape at 16-B lanes 3.19 vs 3.17).
int g_x16_step = 0;
constexpr int64_t kSmallRows16 = 65536;

namespace {

constexpr int kBlock16 = 256;

// V 16-bit elements of one lane, as loaded.
template <int V> struct Raw16 { typedef uint32_t __attribute__((ext_vector_type(V / 2))) T; };
template <> struct Raw16<2> { typedef uint32_t T; };
template <> struct Raw16<1> { typedef uint16_t T; };

// acc[v] = fmaf(s, float(x[v]), acc[v]) for the lane's V elements.
template <typename XT, int V>
__device__ __forceinline__ void fma16(float (&acc)[V], float s, const typename Raw16<V>::T &x) {
    if constexpr (V == 1) {
        acc[0] = __builtin_fmaf(s, widen16<XT>(x), acc[0]);
    } else if constexpr (V == 2) {
        float lo, hi;
        widen16x2<XT>(x, lo, hi);
        acc[0] = __builtin_fmaf(s, lo, acc[0]);
        acc[1] = __builtin_fmaf(s, hi, acc[1]);
    } else {
#pragma unroll
        for (int d = 0; d < V / 2; ++d) {
            float lo, hi;
            widen16x2<XT>(x[d], lo, hi);
            acc[2 * d] = __builtin_fmaf(s, lo, acc[2 * d]);
            acc[2 * d + 1] = __builtin_fmaf(s, hi, acc[2 * d + 1]);
        }
    }
}

// The lane's V chain values into Y at feature f: one vector store (rounded
// and packed for a 16-bit Y) or, where Y's layout does not allow it, one
// element at a time and never past F.
template <typename YT, int V>
__device__ __forceinline__ void store16(YT *__restrict__ yrow, int f, int F, bool vec_store,
                                        const float (&acc)[V]) {
    if (!vec_store) {
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (f + v < F) store_elem<YT>(yrow + f + v, acc[v]);
        return;
    }
    if constexpr (sizeof(YT) == 4) {
        constexpr int W = V < 4 ? V : 4;  // floats per store
        using VT = typename Vec<W>::T;
#pragma unroll
        for (int q = 0; q < V / W; ++q) {
            VT o;
#pragma unroll
            for (int v = 0; v < W; ++v) set_elem<W>(o, v, acc[q * W + v]);
            *reinterpret_cast<VT *>(yrow + f + q * W) = o;
        }
    } else if constexpr (V == 1) {
        store_elem<YT>(yrow + f, acc[0]);
    } else {
        typename Raw16<V>::T o;
        if constexpr (V == 2) {
            o = round16<YT>(acc[0]) | (round16<YT>(acc[1]) << 16);
        } else {
#pragma unroll
            for (int d = 0; d < V / 2; ++d)
                o[d] = round16<YT>(acc[2 * d]) | (round16<YT>(acc[2 * d + 1]) << 16);
        }
        *reinterpret_cast<typename Raw16<V>::T *>(yrow + f) = o;
    }
}

// row_chunks_pipe (spmm.hip) for one V-element vector per lane of 16-bit X:
// the X segments of step s+1 (U nonzeros) are issued before the FMAs of step
// s; the (col, val) block of the next 64 nonzeros is loaded one block ahead;
// loads are never predicated (indices past the row clamp to its last nonzero)
// and only the FMAs are skipped, with wave-uniform branches.  Same FMA order.
template <typename XT, typename YT, int V, int U, bool O32>
__device__ __forceinline__ void row16_pipe(const int *__restrict__ col,
                                           const float *__restrict__ val, int k0, int k1,
                                           const char *__restrict__ Xb, int64_t row_bytes,
                                           YT *__restrict__ yrow, int F, int f, bool vec_store,
                                           int lane, bool accum) {
    using RT = typename Raw16<V>::T;
    constexpr int kSteps = kWave / U;  // steps per 64-nonzero block
    static_assert(kWave % U == 0 && kSteps % 2 == 0, "U must divide 64 into an even count");
    if (accum && k1 == k0) return;  // nothing to add: the row keeps its partial chains
    const bool ok = f < F;
    const uint32_t boff = uint32_t(gather_col(f, F, V)) * 2u;  // idle lanes: lane_lines.h
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0f;
    if constexpr (sizeof(YT) == 4) {  // continue the chains an earlier pass stored (fp32 Y only)
        if (accum && ok) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (f + v < F) acc[v] = load_elem<YT>(yrow + f + v);
        }
    }
    if (k1 > k0) {
        const int last = k1 - 1;
        // (col, val) of blocks b (A) and b+1 (B); clamped, never predicated
        int colA = col[min(k0 + lane, last)];
        float valA = val[min(k0 + lane, last)];
        int colB = col[min(k0 + kWave + lane, last)];
        float valB = val[min(k0 + kWave + lane, last)];
        RT xv[2][U];
        float vv[2][U];
        auto issue = [&](int base, int i, int colr, float valr, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = min(base + i * U + u, last);
                const int l = (k - base) & (kWave - 1);  // clamped past the row: any lane
                                                         // of colr holds a valid column
                const int cj = __builtin_amdgcn_readlane(colr, l);
                vv[buf][u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), l));
                if constexpr (O32)  // X spans < 4 GiB: 32-bit row offsets
                    xv[buf][u] = *reinterpret_cast<const RT *>(
                        Xb + (__umul24((uint32_t)cj, (uint32_t)row_bytes) + boff));
                else
                    xv[buf][u] = *reinterpret_cast<const RT *>(Xb + (int64_t)cj * row_bytes + boff);
            }
        };
        issue(k0, 0, colA, valA, 0);
        for (int base = k0;; base += kWave) {
#pragma unroll
            for (int i = 0; i < kSteps; ++i) {
                const int cur = base + i * U;
                if (cur > last) break;  // uniform; the step issued for it is dropped
                if (i + 1 < kSteps)
                    issue(base, i + 1, colA, valA, (i + 1) & 1);
                else  // first step of the next block, from its prefetched (col, val)
                    issue(base + kWave, 0, colB, valB, 0);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (cur + u <= last) fma16<XT, V>(acc, vv[i & 1][u], xv[i & 1][u]);
                }
            }
            if (base + kWave > last) break;
            colA = colB;
            valA = valB;
            colB = col[min(base + 2 * kWave + lane, last)];
            valB = val[min(base + 2 * kWave + lane, last)];
        }
    }
    if (ok) store16<YT, V>(yrow, f, F, vec_store, acc);
}

// Nonzeros per step (two steps in flight): 16-B lanes hold 8 x 4 registers of
// gathered X per step, narrower lanes go deeper.
constexpr int light_u(int V) { return V >= 4 ? 8 : 16; }

// Grid: x = work items of one feature slice (heavy sub-chunk items first,
// heaviest row first, then the light rows in the plan's order), y = slice.
template <typename XT, typename YT, int V, bool O32, int U = light_u(V)>
__global__ __launch_bounds__(256) void spmm16_kernel(
    const int *__restrict__ row_ptr, const int *__restrict__ col, const float *__restrict__ val,
    const XT *__restrict__ X, int64_t ldx, YT *__restrict__ Y, int64_t ldy, int row_begin,
    int n_items, int F, int vec_store, const int *__restrict__ heavy_rows, int n_heavy,
    int heavy_threshold, int accum, const int *__restrict__ light_rows) {
    constexpr int VH = V < 4 ? V : 4;  // heavy lanes' vector width (8-B lanes)
    constexpr int kSub = V / VH;       // 64*VH-element sub-chunks per slice
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(
        (int)(blockIdx.x * (kBlock16 / kWave) + (threadIdx.x / kWave)));
    const int f_slice = (int)blockIdx.y * (kWave * V);
    const char *Xb = reinterpret_cast<const char *>(X);
    const int64_t row_bytes = ldx * 2;
    const int n_heavy_items = n_heavy * kSub;
    if (wave < n_heavy_items) {
        const int h = wave / kSub;
        const int f_sub = f_slice + (wave - h * kSub) * (kWave * VH);
        if (f_sub >= F) return;
        const int row = heavy_rows[h];
        row16_pipe<XT, YT, VH, 16, O32>(col, val, row_ptr[row], row_ptr[row + 1], Xb, row_bytes,
                                        Y + (int64_t)(row - row_begin) * ldy, F,
                                        f_sub + lane * VH, vec_store != 0, lane, accum != 0);
        return;
    }
    const int w = wave - n_heavy_items;
    if (w >= n_items) return;
    const int row = light_rows ? light_rows[w] : row_begin + w;
    const int k0 = row_ptr[row], k1 = row_ptr[row + 1];
    if (k1 - k0 > heavy_threshold) return;  // done as a heavy item or by the hub kernel
    row16_pipe<XT, YT, V, U, O32>(col, val, k0, k1, Xb, row_bytes,
                                           Y + (int64_t)(row - row_begin) * ldy, F,
                                           f_slice + lane * V, vec_store != 0, lane, accum != 0);
}

template <typename XT, typename YT, int HC, int NL>
__global__ __launch_bounds__(64 * (NL + 1)) void spmm16_hub_kernel(
    const int *__restrict__ row_ptr, const int *__restrict__ col, const float *__restrict__ val,
    const XT *__restrict__ X, int64_t ldx, YT *__restrict__ Y, int64_t ldy, int row_begin, int F,
    const int *__restrict__ hub_rows, int n_chunks, int accum) {
    hub_body<HC, NL, kHubInstr, XT, YT>((int)blockIdx.x, row_ptr, col, val, X, ldx, Y, ldy,
                                        row_begin, F, hub_rows, n_chunks, accum);
}

struct Args16 {
    const int *row_ptr;
    const int *col;
    const float *val;
    const void *X;
    int64_t ldx;
    void *Y;
    int64_t ldy;
    int row_begin, n_rows, F;
    const int *heavy_rows;
    int n_heavy, heavy_threshold, accum;
    const int *light_rows;
    int n_light;
    uint32_t flags;
};

// Widest lane vector X allows: rows and base aligned to it, and the lane
// that holds column F - 1 reads no column the caller did not declare readable.
int pick_vec16(const Args16 &a) {
    const uintptr_t xa = reinterpret_cast<uintptr_t>(a.X);
    const int cap = g_x16_vec ? g_x16_vec : (a.F > 8 * kWave ? 4 : 8);
    for (int V : {8, 4, 2}) {
        if (V > cap) continue;
        const int64_t FV = ((int64_t)a.F + V - 1) / V * V;
        if (a.ldx % V == 0 && xa % (2 * V) == 0 && FV <= a.ldx &&
            (FV == a.F || (a.flags & SGC_SPMM_X_PADDED)))
            return V;
    }
    return 1;
}

template <typename YT>
int vec_store16(const Args16 &a, int V) {
    // the heavy items store min(V, 4)-element vectors at multiples of it
    const int64_t FV = ((int64_t)a.F + V - 1) / V * V;
    const uintptr_t ya = reinterpret_cast<uintptr_t>(a.Y);
    const int W = sizeof(YT) == 4 ? std::min(V, 4) : V;  // elements per store instruction
    return a.ldy % V == 0 && ya % (sizeof(YT) * W) == 0 && FV <= a.ldy &&
           (FV == a.F || (a.flags & SGC_SPMM_Y_PADDED));
}

template <typename XT, typename YT, int V, bool O32, int U = light_u(V)>
hipError_t launch16(const Args16 &a, hipStream_t s) {
    constexpr int kSub = V / (V < 4 ? V : 4);
    const int n_items = a.light_rows ? a.n_light : a.n_rows;
    const int64_t waves = (int64_t)a.n_heavy * kSub + n_items;
    const int64_t blocks = (waves + kBlock16 / kWave - 1) / (kBlock16 / kWave);
    const int64_t slices = ((int64_t)a.F + kWave * V - 1) / (kWave * V);
    if (blocks >= INT32_MAX || slices >= 65536) return hipErrorInvalidValue;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL((spmm16_kernel<XT, YT, V, O32, U>), dim3((unsigned)blocks, (unsigned)slices),
                       dim3(kBlock16), 0, s, a.row_ptr, a.col, a.val,
                       static_cast<const XT *>(a.X), a.ldx, static_cast<YT *>(a.Y), a.ldy,
                       a.row_begin, n_items, a.F, vec_store16<YT>(a, V), a.heavy_rows, a.n_heavy,
                       a.heavy_threshold, a.accum, a.light_rows);
    return hipGetLastError();
}

template <typename XT, typename YT>
hipError_t launch16_v(const Args16 &a, hipStream_t s) {
    const int V = pick_vec16(a);
    // 32-bit row offsets (one 24-bit multiply per gathered row): the caller
    // vouches that X has < 2^24 rows and spans < 4 GiB
    const bool o32 = (a.flags & SGC_SPMM_X_UNDER_4G) && a.ldx * 2 < (int64_t(1) << 24);
    const int step = g_x16_step ? g_x16_step : (a.n_rows < kSmallRows16 ? 4 : 8);
    if (V == 8 && step == 4)
        return o32 ? launch16<XT, YT, 8, true, 4>(a, s) : launch16<XT, YT, 8, false, 4>(a, s);
    if (V == 8) return o32 ? launch16<XT, YT, 8, true>(a, s) : launch16<XT, YT, 8, false>(a, s);
    if (V == 4) return o32 ? launch16<XT, YT, 4, true>(a, s) : launch16<XT, YT, 4, false>(a, s);
    if (V == 2) return launch16<XT, YT, 2, false>(a, s);
    return launch16<XT, YT, 1, false>(a, s);
}

template <typename XT, typename YT>
hipError_t launch16_hub(const Args16 &a, const int *hub_rows, int64_t n_hub, int hc, int nl,
                        hipStream_t s) {
    const int n_chunks = (a.F + hc - 1) / hc;
    const dim3 grid((unsigned)(n_hub * n_chunks));
#define SGC_LAUNCH_HUB16(HCV, NLV)                                                              \
    hipLaunchKernelGGL((spmm16_hub_kernel<XT, YT, HCV, NLV>), grid, dim3(64 * (NLV + 1)), 0, s, \
                       a.row_ptr, a.col, a.val, static_cast<const XT *>(a.X), a.ldx,            \
                       static_cast<YT *>(a.Y), a.ldy, a.row_begin, a.F, hub_rows, n_chunks,     \
                       a.accum)
    if (hc == 32) {
        if (nl == 7) SGC_LAUNCH_HUB16(32, 7);
        else SGC_LAUNCH_HUB16(32, 15);
    } else {
        if (nl == 7) SGC_LAUNCH_HUB16(64, 7);
        else SGC_LAUNCH_HUB16(64, 15);
    }
#undef SGC_LAUNCH_HUB16
    return hipGetLastError();
}

template <typename XT, typename YT>
int run16(Args16 a, int64_t n_hub, hipStream_t stream) {
    const bool hub_only = (a.flags & SGC_SPMM_HUB_ONLY) != 0;
    hipStream_t light_stream = stream;
    void *side = nullptr;
    if (n_hub > 0) {
        SGC_REQUIRE(n_hub * (((int64_t)a.F + 31) / 32) < (int64_t)INT32_MAX, SGC_ERANGE,
                    "spmm_x16: too many hub items");
        // a 64-element chunk of a nonzero is one 128-B line of a 16-bit row
        const int64_t hc_t = get_tuning("hub_chunk"), hs_t = get_tuning("hub_stream");
        const int hc = hc_t ? (int)hc_t : 64;
        const int nl = get_tuning("hub_loaders") == 7 ? 7 : 15;
        const bool serial = hs_t == 2 || (hs_t == 0 && (a.flags & SGC_SPMM_HUB_SERIAL));
        // the hub kernel on the caller's stream; the light kernel beside it
        // on the side stream unless the launch is serial (as launch_spmm)
        if (!hub_only && !serial) {
            const int rc = fork_light_stream(stream, &light_stream, &side);
            if (rc != SGC_OK) return rc;
        }
        const hipError_t e = launch16_hub<XT, YT>(a, a.heavy_rows, n_hub, hc, nl, stream);
        if (e != hipSuccess) {
            if (side) (void)join_light_stream(side, stream);
            set_error("spmm_x16 hub launch failed: %s", hipGetErrorString(e));
            return SGC_EHIP;
        }
        a.heavy_rows += n_hub;
        a.n_heavy -= (int)n_hub;
        if (hub_only) return SGC_OK;
    }
    const hipError_t e = launch16_v<XT, YT>(a, light_stream);
    if (side) {
        const int rc = join_light_stream(side, stream);
        if (rc != SGC_OK) return rc;
    }
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "spmm_x16 launch failed: %s", hipGetErrorString(e));
    return SGC_OK;
}

}  // namespace

int launch_spmm_x16(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                    int64_t row_begin, int64_t row_end, const void *X, int32_t x_dtype,
                    int64_t ldx, void *Y, int32_t y_dtype, int64_t ldy, int64_t F,
                    const int32_t *heavy_rows, int64_t n_heavy, int64_t n_hub,
                    int32_t heavy_threshold, uint32_t flags, hipStream_t stream) {
    SGC_REQUIRE(x_dtype == SGC_DTYPE_BF16 || x_dtype == SGC_DTYPE_F16, SGC_EINVAL,
                "spmm_x16: x_dtype %d is neither SGC_DTYPE_BF16 nor SGC_DTYPE_F16", (int)x_dtype);
    SGC_REQUIRE(y_dtype == x_dtype || y_dtype == SGC_DTYPE_F32, SGC_EINVAL,
                "spmm_x16: y_dtype %d must be x_dtype (%d) or SGC_DTYPE_F32", (int)y_dtype,
                (int)x_dtype);
    SGC_REQUIRE(!(flags & SGC_SPMM_ACCUMULATE) || y_dtype == SGC_DTYPE_F32, SGC_EINVAL,
                "spmm_x16: SGC_SPMM_ACCUMULATE needs an fp32 Y (a chain continued from a "
                "16-bit store would not be exact)");
    SGC_REQUIRE(row_ptr && X && Y, SGC_EINVAL, "spmm_x16: null pointer");
    SGC_REQUIRE(row_begin >= 0 && row_end >= row_begin && row_end < INT32_MAX, SGC_ERANGE,
                "spmm_x16: bad row range [%lld, %lld)", (long long)row_begin, (long long)row_end);
    SGC_REQUIRE(F > 0 && F < (1 << 24), SGC_EINVAL, "spmm_x16: bad feature count %lld",
                (long long)F);
    SGC_REQUIRE(ldx >= F && ldy >= F, SGC_EINVAL, "spmm_x16: ldx/ldy (%lld/%lld) < F (%lld)",
                (long long)ldx, (long long)ldy, (long long)F);
    SGC_REQUIRE(reinterpret_cast<uintptr_t>(X) % 2 == 0 &&
                    reinterpret_cast<uintptr_t>(Y) % (y_dtype == SGC_DTYPE_F32 ? 4 : 2) == 0,
                SGC_EINVAL, "spmm_x16: X / Y not aligned to their element size");
    SGC_REQUIRE(n_heavy >= 0 && (n_heavy == 0 || heavy_rows), SGC_EINVAL, "spmm_x16: bad plan");
    const int64_t n_rows = row_end - row_begin;
    if (n_rows == 0) return SGC_OK;
    // the plan prologue shared with launch_spmm (no non-empty or wide counts here)
    SpmmPlan pl;
    char err[160];
    const int rc = spmm_plan_prologue("spmm_x16", n_rows, heavy_rows != nullptr, n_heavy, n_hub,
                                      heavy_threshold, flags, -1, -1, 0, 0, &pl, err, sizeof(err));
    SGC_REQUIRE(rc == SGC_OK, rc, "%s", err);
    const int *light_rows = pl.light_offset >= 0 ? heavy_rows + pl.light_offset : nullptr;
    const int64_t n_light = pl.n_light;
    if (heavy_rows) heavy_rows += pl.heavy_skip;
    n_heavy = pl.n_heavy;
    n_hub = pl.n_hub;
    heavy_threshold = pl.heavy_threshold;
    if ((flags & SGC_SPMM_HUB_ONLY) && n_hub == 0) return SGC_OK;
    SGC_REQUIRE(n_heavy * 2 + n_rows < (int64_t)INT32_MAX, SGC_ERANGE,
                "spmm_x16: too many work items");
    const Args16 a{row_ptr, col_idx, val, X, ldx, Y, ldy, (int)row_begin, (int)n_rows, (int)F,
                   heavy_rows, (int)n_heavy, heavy_threshold,
                   (flags & SGC_SPMM_ACCUMULATE) ? 1 : 0, light_rows, (int)n_light, flags};
    const bool y32 = y_dtype == SGC_DTYPE_F32;
    if (x_dtype == SGC_DTYPE_BF16)
        return y32 ? run16<bf16_t, float>(a, n_hub, stream) : run16<bf16_t, bf16_t>(a, n_hub, stream);
    return y32 ? run16<f16_t, float>(a, n_hub, stream) : run16<f16_t, f16_t>(a, n_hub, stream);
}

}  // namespace sgc
