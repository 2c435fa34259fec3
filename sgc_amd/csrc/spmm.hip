// spmm.hip -- CSR SpMM  Y = S[rows] . X  for gfx950 (MI355X), bit-exact with
// the reference CPU path (torch.spmm at the reference's utils.py:95).
//
// Numerical contract (pinned by tests/golden): every output
// element is ONE sequential fp32 FMA chain over its row's nonzeros in CSR
// order, starting from +0.0f.  So a lane owns features and walks the row's
// nonzeros in order; no (row, feature) sum is ever split across lanes or
// waves.  The one split is across launches, in order: with
// SGC_SPMM_ACCUMULATE a launch over column block g of S continues each chain
// from the fp32 value block g-1's launch stored (an exact round trip), so the
// passes over blocks 0, 1, ... of a row's CSR-ordered nonzeros are one chain.
//
// Mapping (one wavefront = 64 lanes per work item):
//   * features are cut into slices of 64*C*V floats (grid y); each slice is
//     a complete pass over S, so the live part of X is N x slice floats (see
//     the kernel comment: Infinity Cache / L2 residency);
//   * light item = one row of one slice: lane l owns the V-float vectors at
//     features (slice*C + c)*64V + l*V, c in [0, C): C*V accumulators/lane;
//     each nonzero's X row segment is read as 64V-float coalesced loads;
//   * heavy item = one 64-float sub-chunk of a row with > heavy_threshold
//     nonzeros: power-law hubs run on 2..C*V waves per slice with UH nonzeros
//     in flight each, scheduled first in their slice (sgc_plan_build sorts
//     them by degree), still one FMA chain per element;
//   * (col, val) of 64 consecutive nonzeros are read with one coalesced
//     256-B load each, then broadcast per nonzero with v_readlane into SGPRs,
//     so the X row base address is wave-uniform;
//   * U nonzeros are in flight per wave before their FMAs (U*C*V registers);
//     TLP (up to 8 waves/SIMD) hides the rest of the HBM/MALL latency.
//
// Lanes beyond F (ragged last chunk) still execute every gather -- no
// exec-mask branches sit in the inner loop -- and are never stored.  They
// gather the last valid vector of their instruction's segment (gather_col,
// lane_lines.h): a 128-B line an active lane of the same instruction reads
// anyway, so the ragged chunk touches no line the result does not need.
#include "common.h"
#include "hub.h"
#include "internal.h"
#include "lane_lines.h"
#include "spmm_schedule.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace sgc {

constexpr int kBlock = 256;  // threads per light/heavy workgroup

// CSR (col, val) loads (streamed once per slice).
template <typename T>
__device__ __forceinline__ T ld_meta(const T *p) {
    return *p;
}

// Software-pipelined form of row_chunks: the X segments of step s+1 (U
// nonzeros) are issued before the FMAs of step s, so a wave always has one
// to two steps of gathers in flight instead of draining to zero between
// steps; the (col, val) block of the next 64 nonzeros is loaded one block
// ahead.  Loads are never predicated (a predicated load's phi copy would
// wait for every load in flight): indices past the row clamp to its last
// nonzero (same lines, no extra traffic) and only the FMAs are skipped, with
// wave-uniform branches.  Same FMA order as row_chunks.
template <int V, int C, int U>
__device__ __forceinline__ void row_chunks_pipe(const int *__restrict__ col,
                                                const float *__restrict__ val, int k0, int k1,
                                                const float *__restrict__ X, int64_t ldx,
                                                float *__restrict__ yrow, int F, int chunk0,
                                                int lane, bool accum) {
    using VT = typename Vec<V>::T;
    constexpr int kSteps = kWave / U;  // steps per 64-nonzero block
    static_assert(kWave % U == 0 && kSteps % 2 == 0, "U must divide 64 into an even count");
    if (accum && k1 == k0) return;  // nothing to add: the row keeps its partial chains
    uint32_t boff[C];
    bool ok[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int f = (chunk0 + c) * (kWave * V) + lane * V;
        ok[c] = f < F;
        boff[c] = uint32_t(gather_col(f, F, V)) * 4u;  // idle lanes: lane_lines.h
    }
    VT acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) set_elem<V>(acc[c], v, 0.0f);
    if (accum) {  // continue the chains an earlier column-block pass stored
        const char *Yr = reinterpret_cast<const char *>(yrow);
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (ok[c]) acc[c] = *reinterpret_cast<const VT *>(Yr + boff[c]);
    }

    if (k1 > k0) {
        const char *Xb = reinterpret_cast<const char *>(X);
        const int64_t row_bytes = ldx * 4;
        const int last = k1 - 1;
        // (col, val) of blocks b (A) and b+1 (B); clamped, never predicated
        int colA = ld_meta(col + min(k0 + lane, last));
        float valA = ld_meta(val + min(k0 + lane, last));
        int colB = ld_meta(col + min(k0 + kWave + lane, last));
        float valB = ld_meta(val + min(k0 + kWave + lane, last));
        VT xv[2][U][C];
        float vv[2][U];
        // step (block base, step i) -> buffer i & 1; lanes of the block in colA/colB
        auto issue = [&](int base, int i, int colr, float valr, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = min(base + i * U + u, last);
                const int l = (k - base) & (kWave - 1);  // clamped past the row: any lane
                                                         // of colr holds a valid column
                const int cj = __builtin_amdgcn_readlane(colr, l);
                vv[buf][u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), l));
                const char *xr = Xb + (int64_t)cj * row_bytes;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    xv[buf][u][c] = *reinterpret_cast<const VT *>(xr + boff[c]);
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
                    if (cur + u <= last) {
#pragma unroll
                        for (int c = 0; c < C; ++c)
#pragma unroll
                            for (int v = 0; v < V; ++v)
                                set_elem<V>(acc[c], v,
                                            __builtin_fmaf(vv[i & 1][u],
                                                           lane_elem<V>(xv[i & 1][u][c], v),
                                                           lane_elem<V>(acc[c], v)));
                    }
                }
            }
            if (base + kWave > last) break;
            colA = colB;
            valA = valB;
            colB = ld_meta(col + min(base + 2 * kWave + lane, last));
            valB = ld_meta(val + min(base + 2 * kWave + lane, last));
        }
    }
    char *Yb = reinterpret_cast<char *>(yrow);
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (ok[c]) *reinterpret_cast<VT *>(Yb + boff[c]) = acc[c];
}

// row_chunks_pipe scheduled like row_pairs_pipe: whole 64-nonzero blocks
// without an exit inside them (the compiler then keeps two steps of gathers
// in flight instead of draining to zero between steps), the last block stops
// at the row's end, the (col, val) block after next is loaded before the
// gathers of the step that starts the next block.  Same FMA order.
template <int V, int C, int U>
__device__ __forceinline__ void row_chunks_pipe2(const int *__restrict__ col,
                                                 const float *__restrict__ val, int k0, int k1,
                                                 const float *__restrict__ X, int64_t ldx,
                                                 float *__restrict__ yrow, int F, int chunk0,
                                                 int lane, bool accum) {
    using VT = typename Vec<V>::T;
    constexpr int kSteps = kWave / U;
    static_assert(kWave % U == 0 && kSteps % 2 == 0, "U must divide 64 into an even count");
    if (accum && k1 == k0) return;
    uint32_t boff[C];
    bool ok[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int f = (chunk0 + c) * (kWave * V) + lane * V;
        ok[c] = f < F;
        boff[c] = uint32_t(gather_col(f, F, V)) * 4u;  // idle lanes: lane_lines.h
    }
    VT acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) set_elem<V>(acc[c], v, 0.0f);
    if (accum) {
        const char *Yr = reinterpret_cast<const char *>(yrow);
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (ok[c]) acc[c] = *reinterpret_cast<const VT *>(Yr + boff[c]);
    }
    if (k1 > k0) {
        const char *Xb = reinterpret_cast<const char *>(X);
        const int64_t row_bytes = ldx * 4;
        const int last = k1 - 1;
        int colA = ld_meta(col + min(k0 + lane, last));
        float valA = ld_meta(val + min(k0 + lane, last));
        int colB = ld_meta(col + min(k0 + kWave + lane, last));
        float valB = ld_meta(val + min(k0 + kWave + lane, last));
        VT xv[2][U][C];
        float vv[2][U];
        auto issue = [&](int base, int i, int colr, float valr, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = min(base + i * U + u, last);
                const int l = (k - base) & (kWave - 1);
                const int cj = __builtin_amdgcn_readlane(colr, l);
                vv[buf][u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), l));
                const char *xr = Xb + (int64_t)cj * row_bytes;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    xv[buf][u][c] = *reinterpret_cast<const VT *>(xr + boff[c]);
            }
        };
        auto step = [&](int base, int i, bool last_block) {
            const int cur = base + i * U;
            if (i + 1 < kSteps) {
                issue(base, i + 1, colA, valA, (i + 1) & 1);
            } else if (!last_block) {
                const int nb2 = base + 2 * kWave;  // the block after next
                const int cN = ld_meta(col + min(nb2 + lane, last));
                const float vN = ld_meta(val + min(nb2 + lane, last));
                issue(base + kWave, 0, colB, valB, 0);
                colA = colB;
                valA = valB;
                colB = cN;
                valB = vN;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (cur + u <= last) {
#pragma unroll
                    for (int c = 0; c < C; ++c)
#pragma unroll
                        for (int v = 0; v < V; ++v)
                            set_elem<V>(acc[c], v,
                                        __builtin_fmaf(vv[i & 1][u],
                                                       lane_elem<V>(xv[i & 1][u][c], v),
                                                       lane_elem<V>(acc[c], v)));
                }
            }
        };
        issue(k0, 0, colA, valA, 0);
        const int nblk = (k1 - k0 + kWave - 1) / kWave;
        int base = k0;
        for (int b = 0; b + 1 < nblk; ++b, base += kWave) {
#pragma unroll
            for (int i = 0; i < kSteps; ++i) step(base, i, false);
        }
#pragma unroll
        for (int i = 0; i < kSteps; ++i)  // no exit: skipped steps fall through
            if (base + i * U <= last) step(base, i, true);
    }
    char *Yb = reinterpret_cast<char *>(yrow);
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (ok[c]) *reinterpret_cast<VT *>(Yb + boff[c]) = acc[c];
}

// Heavy row of the multi-row kernel, two nonzeros per load instruction: lanes
// 0-31 gather nonzero k's X segment, lanes 32-63 nonzero k+1's (16-B lanes,
// up to 128 floats per half), so one global_load_dwordx4 moves up to 1 KB
// (a one-row-per-instruction wave moves at most half that, and only the row
// width -- 304 B at a 76-float feature block).  v_permlane32_swap then gives
// every lane both values of its features (lo = x_k, hi = x_k+1) and the chain
// takes them in order, acc = fma(v_k, x_k, acc); acc = fma(v_k+1, x_k+1, acc):
// the same sequential FMA chain per element as one nonzero at a time (both
// halves compute it; the low half stores).  U pairs per step, two steps in
// flight (2U nonzeros each); (col, val) of 64 consecutive nonzeros in one VGPR
// per lane, the next block loaded one ahead.  Indices past the row clamp to
// its last nonzero (never out of bounds) and their FMAs are skipped.
constexpr int kPairsU = 4;  // nonzero pairs per step (8 nonzeros; 16 in flight)

// Schedule: every 64-nonzero block but the last runs all its steps (no exit
// inside a block, so the compiler's wait counts keep two steps in flight
// instead of draining the loads at every block -- with per-step exits they
// did), the last block stops at the row's end; the (col, val) block after
// next is loaded before the gathers of the step that starts the next block.
// Reddit shape K=2: 9.01 -> 8.94 ms, bit-identical (profiles/r03/s5/pairs.log).
//
// TR (transposed pairs, heavy_pairs bit 16): one v_permlane32_swap per two
// registers instead -- (r0, r2) and (r1, r3) -- leaves lane (h, j) (h = lane
// >= 32) with features 4j+2h, 4j+2h+1 of both nonzeros, so each lane runs
// two chains (its two features) at one FMA per nonzero each: two swaps and
// four FMAs per pair where the untransposed form spends four and eight (both
// halves computing every chain); every lane stores its two features.
template <int U, bool O32, bool TR = false>
__device__ __forceinline__ void row_pairs_pipe(const int *__restrict__ col,
                                               const float *__restrict__ val, int k0, int k1,
                                               const float *__restrict__ X, int64_t ldx,
                                               float *__restrict__ yrow, int F, int f_lane,
                                               int f_end, bool vec_store, int lane,
                                               bool accum) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int kPairs = kWave / (2 * U);  // steps per 64-nonzero block
    static_assert(kWave % (2 * U) == 0 && kPairs % 2 == 0, "2U must divide 64 into an even count");
    if (accum && k1 == k0) return;
    typedef float f2 __attribute__((ext_vector_type(2)));
    const bool hi = lane >= 32;
    // f_end: where the computed columns of this item stop (a multiple of 4)
    const bool lane_ok = f_lane < f_end;
    const uint32_t boff = uint32_t(gather_col(f_lane, f_end, 4)) * 4u;  // idle lanes: lane_lines.h
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    f2 acc2 = {0.0f, 0.0f};           // TR: features fo, fo + 1
    const int fo = f_lane + (hi ? 2 : 0);
    if (accum && lane_ok) {
        // !vec_store: a caller's rows (4-B aligned, nothing readable from
        // column F on) -- still one access per lane (load_upto / store_upto)
        if constexpr (TR) {
            if (vec_store)
                acc2 = *reinterpret_cast<const f2 *>(yrow + fo);
            else
                acc2 = load_upto<2>(yrow, fo, F);
        } else if (vec_store) {
            acc = *reinterpret_cast<const f4 *>(yrow + f_lane);
        } else {
            acc = load_upto<4>(yrow, f_lane, F);
        }
    }
    if (k1 > k0) {
        const char *Xb = reinterpret_cast<const char *>(X);
        const int64_t row_bytes = ldx * 4;
        const int last = k1 - 1;
        int colA = ld_meta(col + min(k0 + lane, last));
        float valA = ld_meta(val + min(k0 + lane, last));
        int colB = ld_meta(col + min(k0 + kWave + lane, last));
        float valB = ld_meta(val + min(k0 + kWave + lane, last));
        f4 xv[2][U];
        float v0[2][U], v1[2][U];
        auto issue = [&](int base, int i, int colr, float valr, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ka = min(base + i * 2 * U + 2 * u, last);
                const int kb = min(ka + 1, last);
                const int la = (ka - base) & (kWave - 1), lb = (kb - base) & (kWave - 1);
                const int ca = __builtin_amdgcn_readlane(colr, la);
                const int cb = __builtin_amdgcn_readlane(colr, lb);
                v0[buf][u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), la));
                v1[buf][u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), lb));
                const int cj = hi ? cb : ca;
                if constexpr (O32)
                    xv[buf][u] = *reinterpret_cast<const f4 *>(
                        Xb + (__umul24((uint32_t)cj, (uint32_t)row_bytes) + boff));
                else
                    xv[buf][u] = *reinterpret_cast<const f4 *>(Xb + (int64_t)cj * row_bytes + boff);
            }
        };
        auto step = [&](int base, int i, bool last_block) {
            const int cur = base + i * 2 * U;
            if (i + 1 < kPairs) {
                issue(base, i + 1, colA, valA, (i + 1) & 1);
            } else if (!last_block) {
                const int nb2 = base + 2 * kWave;  // the block after next
                const int cN = ld_meta(col + min(nb2 + lane, last));
                const float vN = ld_meta(val + min(nb2 + lane, last));
                issue(base + kWave, 0, colB, valB, 0);
                colA = colB;
                valA = valB;
                colB = cN;
                valB = vN;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ka = cur + 2 * u;
                if (ka > last) break;  // uniform
                if constexpr (TR) {
                    const f4 x = xv[i & 1][u];
                    const auto s02 = __builtin_amdgcn_permlane32_swap(
                        __float_as_uint(x[0]), __float_as_uint(x[2]), false, false);
                    const auto s13 = __builtin_amdgcn_permlane32_swap(
                        __float_as_uint(x[1]), __float_as_uint(x[3]), false, false);
                    acc2[0] = __builtin_fmaf(v0[i & 1][u], __uint_as_float(s02[0]), acc2[0]);
                    acc2[1] = __builtin_fmaf(v0[i & 1][u], __uint_as_float(s13[0]), acc2[1]);
                    if (ka + 1 <= last) {
                        acc2[0] = __builtin_fmaf(v1[i & 1][u], __uint_as_float(s02[1]), acc2[0]);
                        acc2[1] = __builtin_fmaf(v1[i & 1][u], __uint_as_float(s13[1]), acc2[1]);
                    }
                    continue;
                }
                f4 xa, xb;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const uint32_t x = __float_as_uint(xv[i & 1][u][v]);
                    const auto t = __builtin_amdgcn_permlane32_swap(x, x, false, false);
                    xa[v] = __uint_as_float(t[0]);
                    xb[v] = __uint_as_float(t[1]);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = __builtin_fmaf(v0[i & 1][u], xa[v], acc[v]);
                if (ka + 1 <= last) {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        acc[v] = __builtin_fmaf(v1[i & 1][u], xb[v], acc[v]);
                }
            }
        };
        issue(k0, 0, colA, valA, 0);
        const int nblk = (k1 - k0 + kWave - 1) / kWave;
        int base = k0;
        for (int b = 0; b + 1 < nblk; ++b, base += kWave) {
#pragma unroll
            for (int i = 0; i < kPairs; ++i) step(base, i, false);
        }
#pragma unroll
        for (int i = 0; i < kPairs; ++i)  // no exit: skipped steps fall through
            if (base + i * 2 * U <= last) step(base, i, true);
    }
    if constexpr (TR) {
        if (lane_ok) {
            if (vec_store)
                *reinterpret_cast<f2 *>(yrow + fo) = acc2;
            else
                store_upto<2>(yrow, fo, F, acc2);
        }
    } else if (!hi && lane_ok) {
        if (vec_store)
            *reinterpret_cast<f4 *>(yrow + f_lane) = acc;
        else
            store_upto<4>(yrow, f_lane, F, acc);
    }
}

// Heavy row of a NARROW launch (at most 64 floats), four nonzeros per load
// instruction: lane group g = lane / 16 gathers nonzero k+g's X segment,
// 16 lanes x V floats (V = 4 / 2 / 1: segments of up to 64 / 32 / 16 floats),
// so one load moves four row segments where pairs move two (at 64 floats
// pairs leave half of each 32-lane half idle, at 32 or 12 floats three
// quarters or more).  What bounds a narrow pass is the load instructions (a
// wave instruction costs the texture unit about the same whether it carries
// two or four segments: scripts/micro/gather_rate.hip, 64 floats 0.42 ms at two
// segments per instruction vs 0.37 at four) and a long row's loads in flight
// (4 x U x 2 here: twice the pairs').  Every lane then needs the four
// nonzeros' values of its features, in order:
//   v_permlane32_swap(x, x) -> t0 = x of lane L mod 32 (group 0 or 1, same
//     16-lane position), t1 = x of lane 32 + L mod 32 (group 2 or 3);
//   v_permlane16_swap(t, t) -> t of lane L & ~16 and of lane L | 16:
//     groups 0, 1 from t0 and 2, 3 from t1 -- in every lane, the same order;
// and the chain takes them in nonzero order: acc = fma(v_k, x_k, acc), ...,
// fma(v_k+3, x_k+3, acc), the same sequential FMA chain per element (all four
// groups compute it; group 0 stores).  The S values and column ids come from
// the 64-nonzero (col, val) block by v_readlane (wave-uniform), the column of
// the lane's own group by two selects.
constexpr int kQuadsU = 4;  // quads per step (16 nonzeros; two steps = 32 in flight)

template <int V, int U, bool O32>
__device__ __forceinline__ void row_quads_pipe(const int *__restrict__ col,
                                               const float *__restrict__ val, int k0, int k1,
                                               const float *__restrict__ X, int64_t ldx,
                                               float *__restrict__ yrow, int F, int f_lane,
                                               int f_end, bool vec_store, int lane,
                                               bool accum) {
    using VT = typename Vec<V>::T;
    constexpr int kSteps = kWave / (4 * U);  // steps per 64-nonzero block
    static_assert(kWave % (4 * U) == 0 && kSteps % 2 == 0, "4U must divide 64 into an even count");
    if (accum && k1 == k0) return;
    const int g = lane >> 4;
    // f_end: where the computed columns stop (a multiple of 4, so of V)
    const bool lane_ok = f_lane < f_end;
    const uint32_t boff = uint32_t(gather_col(f_lane, f_end, V)) * 4u;  // idle lanes: lane_lines.h
    VT acc;
#pragma unroll
    for (int v = 0; v < V; ++v) set_elem<V>(acc, v, 0.0f);
    if (accum && lane_ok) {
        if (vec_store)
            acc = *reinterpret_cast<const VT *>(yrow + f_lane);
        else
            acc = load_upto<V>(yrow, f_lane, F);
    }
    if (k1 > k0) {
        const char *Xb = reinterpret_cast<const char *>(X);
        const int64_t row_bytes = ldx * 4;
        const int last = k1 - 1;
        int colA = ld_meta(col + min(k0 + lane, last));
        float valA = ld_meta(val + min(k0 + lane, last));
        int colB = ld_meta(col + min(k0 + kWave + lane, last));
        float valB = ld_meta(val + min(k0 + kWave + lane, last));
        VT xv[2][U];
        float vq[2][U][4];
        auto issue = [&](int base, int i, int colr, float valr, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kq = base + i * 4 * U + 4 * u;
                int c[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int l = (min(kq + j, last) - base) & (kWave - 1);
                    c[j] = __builtin_amdgcn_readlane(colr, l);
                    vq[buf][u][j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), l));
                }
                const int c01 = (g & 1) ? c[1] : c[0];
                const int c23 = (g & 1) ? c[3] : c[2];
                const int cj = (g & 2) ? c23 : c01;
                if constexpr (O32)
                    xv[buf][u] = *reinterpret_cast<const VT *>(
                        Xb + (__umul24((uint32_t)cj, (uint32_t)row_bytes) + boff));
                else
                    xv[buf][u] = *reinterpret_cast<const VT *>(Xb + (int64_t)cj * row_bytes + boff);
            }
        };
        auto step = [&](int base, int i, bool last_block) {
            const int cur = base + i * 4 * U;
            if (i + 1 < kSteps) {
                issue(base, i + 1, colA, valA, (i + 1) & 1);
            } else if (!last_block) {
                const int nb2 = base + 2 * kWave;  // the block after next
                const int cN = ld_meta(col + min(nb2 + lane, last));
                const float vN = ld_meta(val + min(nb2 + lane, last));
                issue(base + kWave, 0, colB, valB, 0);
                colA = colB;
                valA = valB;
                colB = cN;
                valB = vN;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kq = cur + 4 * u;
                if (kq > last) break;  // uniform
                const int n_here = min(4, last - kq + 1);  // uniform
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const uint32_t x = __float_as_uint(lane_elem<V>(xv[i & 1][u], v));
                    const auto t = __builtin_amdgcn_permlane32_swap(x, x, false, false);
                    const auto p = __builtin_amdgcn_permlane16_swap(t[0], t[0], false, false);
                    const auto q = __builtin_amdgcn_permlane16_swap(t[1], t[1], false, false);
                    float a = lane_elem<V>(acc, v);
                    a = __builtin_fmaf(vq[i & 1][u][0], __uint_as_float(p[0]), a);
                    if (n_here > 1) a = __builtin_fmaf(vq[i & 1][u][1], __uint_as_float(p[1]), a);
                    if (n_here > 2) a = __builtin_fmaf(vq[i & 1][u][2], __uint_as_float(q[0]), a);
                    if (n_here > 3) a = __builtin_fmaf(vq[i & 1][u][3], __uint_as_float(q[1]), a);
                    set_elem<V>(acc, v, a);
                }
            }
        };
        issue(k0, 0, colA, valA, 0);
        const int nblk = (k1 - k0 + kWave - 1) / kWave;
        int base = k0;
        for (int b = 0; b + 1 < nblk; ++b, base += kWave) {
#pragma unroll
            for (int i = 0; i < kSteps; ++i) step(base, i, false);
        }
#pragma unroll
        for (int i = 0; i < kSteps; ++i)  // no exit: skipped steps fall through
            if (base + i * 4 * U <= last) step(base, i, true);
    }
    if (g == 0 && lane_ok) {
        if (vec_store)
            *reinterpret_cast<VT *>(yrow + f_lane) = acc;
        else
            store_upto<V>(yrow, f_lane, F, acc);
    }
}

// Heavy row of a 33..64-float launch, four nonzeros per load, TRANSPOSED: lane
// (g, j) (g = lane / 16, j = lane & 15) gathers floats 4j..4j+3 of nonzero
// k+g's segment -- one load moves four 256-B segments, as the light rows' do
// at this width -- and then a 4 x 4 transpose across the four lane groups
// (two v_permlane32_swap: g <-> g^2, two v_permlane16_swap: g <-> g^1) leaves
// lane (g, j) with feature 4j+g of the four nonzeros, in nonzero order:
//   after the 32-swaps (r0,r2), (r1,r3): g < 2 holds f0,f1 of nonzeros g, g+2;
//     g >= 2 holds f2,f3 of nonzeros g-2, g;
//   after the 16-swaps (r0,r1), (r2,r3): r0..r3 = feature 4j+g of nonzeros
//     k..k+3.
// Each lane then runs ONE chain (its feature) with one FMA per nonzero:
// four swaps + four FMAs per four nonzeros, where row_quads_pipe at V = 4
// spends twelve permutes and sixteen FMAs (every group recomputing every
// chain) -- the reason it lost to the pairs at 48-64 floats.  The chain is
// the same sequential fmaf chain per element; every lane stores its feature.
template <int U, bool O32>
__device__ __forceinline__ void row_quadsT_pipe(const int *__restrict__ col,
                                                const float *__restrict__ val, int k0, int k1,
                                                const float *__restrict__ X, int64_t ldx,
                                                float *__restrict__ yrow, int F, int f_lane,
                                                int f_end, int lane, bool accum) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int kSteps = kWave / (4 * U);  // steps per 64-nonzero block
    static_assert(kWave % (4 * U) == 0 && kSteps % 2 == 0, "4U must divide 64 into an even count");
    if (accum && k1 == k0) return;
    const int g = lane >> 4;
    const int fo = f_lane + g;  // this lane's output feature
    // f_end: where the computed columns stop (a multiple of 4)
    const bool lane_ok = f_lane < f_end;
    const bool own = lane_ok && fo < F;
    const uint32_t boff = uint32_t(gather_col(f_lane, f_end, 4)) * 4u;  // idle lanes: lane_lines.h
    float acc = 0.0f;
    if (accum && own) acc = yrow[fo];
    if (k1 > k0) {
        const char *Xb = reinterpret_cast<const char *>(X);
        const int64_t row_bytes = ldx * 4;
        const int last = k1 - 1;
        int colA = ld_meta(col + min(k0 + lane, last));
        float valA = ld_meta(val + min(k0 + lane, last));
        int colB = ld_meta(col + min(k0 + kWave + lane, last));
        float valB = ld_meta(val + min(k0 + kWave + lane, last));
        f4 xv[2][U];
        float vq[2][U][4];
        auto issue = [&](int base, int i, int colr, float valr, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kq = base + i * 4 * U + 4 * u;
                int c[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int l = (min(kq + j, last) - base) & (kWave - 1);
                    c[j] = __builtin_amdgcn_readlane(colr, l);
                    vq[buf][u][j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(valr), l));
                }
                const int c01 = (g & 1) ? c[1] : c[0];
                const int c23 = (g & 1) ? c[3] : c[2];
                const int cj = (g & 2) ? c23 : c01;
                if constexpr (O32)
                    xv[buf][u] = *reinterpret_cast<const f4 *>(
                        Xb + (__umul24((uint32_t)cj, (uint32_t)row_bytes) + boff));
                else
                    xv[buf][u] = *reinterpret_cast<const f4 *>(Xb + (int64_t)cj * row_bytes + boff);
            }
        };
        auto step = [&](int base, int i, bool last_block) {
            const int cur = base + i * 4 * U;
            if (i + 1 < kSteps) {
                issue(base, i + 1, colA, valA, (i + 1) & 1);
            } else if (!last_block) {
                const int nb2 = base + 2 * kWave;  // the block after next
                const int cN = ld_meta(col + min(nb2 + lane, last));
                const float vN = ld_meta(val + min(nb2 + lane, last));
                issue(base + kWave, 0, colB, valB, 0);
                colA = colB;
                valA = valB;
                colB = cN;
                valB = vN;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kq = cur + 4 * u;
                if (kq > last) break;  // uniform
                const int n_here = min(4, last - kq + 1);  // uniform
                const f4 x = xv[i & 1][u];
                const auto s02 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[0]),
                                                                  __float_as_uint(x[2]), false, false);
                const auto s13 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[1]),
                                                                  __float_as_uint(x[3]), false, false);
                const auto t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
                const auto t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
                acc = __builtin_fmaf(vq[i & 1][u][0], __uint_as_float(t01[0]), acc);
                if (n_here > 1) acc = __builtin_fmaf(vq[i & 1][u][1], __uint_as_float(t01[1]), acc);
                if (n_here > 2) acc = __builtin_fmaf(vq[i & 1][u][2], __uint_as_float(t23[0]), acc);
                if (n_here > 3) acc = __builtin_fmaf(vq[i & 1][u][3], __uint_as_float(t23[1]), acc);
            }
        };
        issue(k0, 0, colA, valA, 0);
        const int nblk = (k1 - k0 + kWave - 1) / kWave;
        int base = k0;
        for (int b = 0; b + 1 < nblk; ++b, base += kWave) {
#pragma unroll
            for (int i = 0; i < kSteps; ++i) step(base, i, false);
        }
#pragma unroll
        for (int i = 0; i < kSteps; ++i)  // no exit: skipped steps fall through
            if (base + i * 4 * U <= last) step(base, i, true);
    }
    if (own) yrow[fo] = acc;
}

// Grid: x = work items of one feature slice, y = slice.  Workgroups are
// dispatched x-fastest, so the chip sweeps the slices one after another and
// only X[:, slice] (N x 64CV floats -- 119 MB at Reddit shape for 128
// floats) is live at a time: it stays in the 256 MB Infinity Cache and far
// more of it in the 4 MB per-XCD L2s than whole 2.4 KB rows would.  Within a
// slice the heavy rows come first (heaviest first), each split into
// 64-float sub-chunks (dword loads, UH nonzeros in flight) so a power-law hub
// is spread over 2C*V waves and finishes inside its slice.
#ifndef SGC_HEAVY_VEC
#define SGC_HEAVY_VEC 2
#endif
constexpr int kFusedHubInstr = 8;  // (see HubShape)

// HF > 0: the serial hub rows fused into the launch (as spmm_rows_kernel's HF).
template <int V, int C, int U, int UH, int HF = 0>
__global__ __launch_bounds__(256) void spmm_csr_kernel(
    const int *__restrict__ row_ptr, const int *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, int64_t ldx, float *__restrict__ Y, int64_t ldy,
    int row_begin, int n_rows, int F, const int *__restrict__ heavy_rows, int n_heavy,
    int heavy_threshold, int accum, int heavy_pairs, const int *__restrict__ hub_rows = nullptr,
    int hub_chunks = 0, int n_hub_blocks = 0) {
    constexpr int VH = (SGC_HEAVY_VEC < V) ? SGC_HEAVY_VEC : V;  // heavy lanes' vector width
    constexpr int kSub = C * V / VH;  // 64*VH-float sub-chunks per slice (heavy items)
    int bx = (int)blockIdx.x;
    if constexpr (HF > 0) {
        if (bx < n_hub_blocks) {  // block-uniform
            if (blockIdx.y == 0)
                hub_body<HF, 3, kFusedHubInstr>(bx, row_ptr, col, val, X, ldx, Y, ldy, row_begin, F, hub_rows,
                                hub_chunks, accum);
            return;
        }
        bx -= n_hub_blocks;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(
        (int)(bx * (blockDim.x / kWave) + (threadIdx.x / kWave)));
    const int slice = blockIdx.y;
    const int n_heavy_items = n_heavy * kSub;
    if (wave < n_heavy_items) {
        const int h = wave / kSub;
        const int sub = slice * kSub + (wave - h * kSub);  // in units of 64*VH floats
        if (sub * kWave * VH >= F) return;
        const int row = heavy_rows[h];
        const int k0 = row_ptr[row], k1 = row_ptr[row + 1];
        if constexpr (V == 4 && VH == 2) {
            if (heavy_pairs & 1) {  // the same 128-float sub-chunk, two nonzeros per load
                const int f = sub * 128 + (lane & 31) * 4;
                row_pairs_pipe<kPairsU, false>(col, val, k0, k1, X, ldx,
                                               Y + (int64_t)(row - row_begin) * ldy, F, f, F,
                                               true, lane, accum != 0);
                return;
            }
        }
        if (heavy_pairs & 2)
            row_chunks_pipe2<VH, 1, UH / VH>(col, val, k0, k1, X, ldx,
                                             Y + (int64_t)(row - row_begin) * ldy, F, sub, lane,
                                             accum != 0);
        else
            row_chunks_pipe<VH, 1, UH / VH>(col, val, k0, k1, X, ldx,
                                            Y + (int64_t)(row - row_begin) * ldy, F, sub, lane,
                                            accum != 0);
        return;
    }
    const int r = wave - n_heavy_items;
    if (r >= n_rows) return;
    const int row = row_begin + r;
    const int k0 = row_ptr[row], k1 = row_ptr[row + 1];
    if (k1 - k0 > heavy_threshold) return;  // done as a heavy item or by the hub kernel
    if (heavy_pairs & 2)
        row_chunks_pipe2<V, C, U>(col, val, k0, k1, X, ldx, Y + (int64_t)r * ldy, F, slice * C,
                                  lane, accum != 0);
    else
        row_chunks_pipe<V, C, U>(col, val, k0, k1, X, ldx, Y + (int64_t)r * ldy, F, slice * C,
                                 lane, accum != 0);
}

// ---------------------------------------------------------------------------
// Multi-row light kernel: LR lanes per row (8..32, a launch parameter), 4
// floats per lane (one global_load_dwordx4), R = 64 / LR rows per wavefront.
// A feature slice is LR * 4 floats: 128 at LR = 32 (2 rows per wave); a
// narrow launch -- a 76-float feature block, a 64-float group -- takes
// LR = width / 4 and a single slice, so up to 64 / LR rows share the wave
// instead of leaving most lanes idle.  (spmm_csr_kernel covers a 128-float
// slice with one row per wave and 8-B lanes: twice the load instructions for
// the same bytes, and at most one row per wave at any width.)
// It computes the columns up to F_load = F rounded up to 4: the engine's own
// 128-B-row buffers hold pad columns (don't-care values, computed like any
// other column, never returned); stores into a caller's buffer stop at F.
//  * each row's next LB (col, val) pairs are staged in a per-wave LDS block
//    (double buffered, loaded one block ahead); a lane reads U = 4 of its
//    row's ids and values with one ds_read_b128 each, a broadcast within the
//    row's LR lanes;
//  * U nonzeros per row per step, two steps in flight (software pipelined);
//  * the rows of one wave have different lengths: the wave runs to the
//    longest; lanes past their row's end re-load their row's last nonzero
//    (same lines, never out of bounds) and skip the FMAs -- still one
//    sequential FMA chain per element in CSR order.
// Heavy items (rows above heavy_threshold) come first in the grid, as in
// spmm_csr_kernel: one wave per 64*VH-float sub-chunk, n_sub per slice (8-B
// lanes at F % 4 != 0, one row per load instruction, twice the loads in
// flight per row; packing heavy rows R per wave like light rows measured 1.7x
// slower on a 76-float slice, profiles/r02/packed_sweep.log).
constexpr int kRowsU = 4;  // nonzeros per row per step (one b128 (col, val) read each)


// Wide item (short_wide): the wave's R = 2 light rows of at most LBW nonzeros,
// carried through EVERY feature slice of the launch by this one wave.  The
// per-slice path pays light_rows -> row_ptr -> (col, val) -> gathers -> FMAs
// -> store once per slice and wave for rows that hold a handful of nonzeros;
// here the first three are read once, the whole row sits in one LDS block
// that is never restaged, and the (slice, step) pairs run as ONE software
// pipeline: step t + 1 -- the next slice's first step when t ends a slice --
// is issued before the FMAs of step t, so the gathers stay in flight across
// the slice boundary.  Every (row, feature) chain is the per-slice path's:
// fmaf in CSR order from +0.0f, or (ACC) from the stored value, loaded ahead
// of the slice's first gathers.  Lane addressing as in the per-slice path:
// gather_col against the current slice's seg_end, stage_index for the
// staging lanes, stores into a caller's rows stop at F.  A row longer than
// LBW (a caller's wrong count) is cut to LBW: wrong values, never a wild
// address.
template <int LBW, bool O32, bool ACC>
__device__ __forceinline__ void wide_rows_body(
    int ww, int wl, int lane, const int *__restrict__ row_ptr, const int *__restrict__ col,
    const float *__restrict__ val, const float *__restrict__ X, int64_t ldx,
    float *__restrict__ Y, int64_t ldy, int row_begin, int n_wide, int F, int F_load,
    int vec_store, int n_slices, const int *__restrict__ wide_rows, int (*s_col)[2][kWave],
    float (*s_val)[2][kWave]) {
    constexpr int V = 4, U = 4, LR = 32, R = kWave / LR, SW = LR * V;
    static_assert(R * LBW <= kWave && LBW % U == 0, "bad wide block");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef int i4 __attribute__((ext_vector_type(4)));
    if (ww * R >= n_wide) return;  // wave-uniform
    const int sub = lane / LR, l = lane - sub * LR;
    const int li = ww * R + sub;
    int r = 0, k0 = 0, len = 0;
    bool mine = false;
    if (li < n_wide) {
        const int row = wide_rows[li];
        r = row - row_begin;
        k0 = row_ptr[row];
        len = min(row_ptr[row + 1] - k0, LBW);
        mine = true;
    }
    const int len0 = __builtin_amdgcn_readlane(len, 0), len1 = __builtin_amdgcn_readlane(len, LR);
    const int n_max = max(len0, len1), n_min = min(len0, len1);
    const int k_max = __builtin_amdgcn_readlane(k0, len1 > len0 ? LR : 0);
    float *yr = Y + (int64_t)r * ldy;
    // accumulate: rows without nonzeros in this pass are neither read into a
    // result nor written
    const bool live = mine && (!ACC || len > 0);
    auto slice_end = [&](int s) { return min(F_load, (s + 1) * SW); };
    auto store = [&](int s, const f4 &a) {
        const int f = s * SW + l * V;
        if (live && f < slice_end(s)) {
            if (vec_store)
                *reinterpret_cast<f4 *>(yr + f) = a;
            else
                store_upto<V>(yr, f, F, a);
        }
    };
    if (n_max == 0) {  // only rows without nonzeros: zeros (a plain launch), or nothing
        if constexpr (!ACC) {
            const f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int s = 0; s < n_slices; ++s) store(s, z);
        }
        return;
    }
    const char *Xb = reinterpret_cast<const char *>(X);
    const int64_t row_bytes = ldx * 4;
    const int lds_row = sub * LBW;
    {   // the rows' (col, val), once: never predicated (stage_index, lane_lines.h);
        // a row without nonzeros stages what the wave's longest row does
        const int k0_s = len > 0 ? k0 : k_max, len_s = len > 0 ? len : n_max;
        const int kk = k0_s + stage_index(0, l, LBW, len_s);
        const int c = col[kk];
        const float v = val[kk];
        if (l < LBW) {
            s_col[wl][0][lds_row + l] = c;
            s_val[wl][0][lds_row + l] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const int nst = (n_max + U - 1) / U;  // steps per slice (wave-uniform)
    const int T = nst * n_slices;
    // idle lanes of a ragged slice stay on a line an active lane reads
    auto slice_col = [&](int s) { return gather_col(s * SW + l * V, slice_end(s), V); };
    f4 xv[2][U];
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, accN = {0.0f, 0.0f, 0.0f, 0.0f};
    int is = 0, ii = 0;  // the issue cursor: (slice, step)
    int col_i = slice_col(0);
    auto issue = [&](int slot) {
        if constexpr (ACC) {
            if (ii == 0) {  // uniform: the slice's stored chains, ahead of its gathers
                // every lane loads (idle lanes their clamped column, lanes
                // without a row the range's first row): nothing predicated
                if (vec_store)
                    accN = *reinterpret_cast<const f4 *>(yr + col_i);
                else  // a caller's rows: nothing readable from column F on
                    accN = load_upto<V>(yr, col_i, F);
            }
        }
        const uint32_t boff = uint32_t(col_i) * 4u;
        const i4 cc = *reinterpret_cast<const i4 *>(&s_col[wl][0][lds_row + ii * U]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (O32)
                xv[slot][u] = *reinterpret_cast<const f4 *>(
                    Xb + (__umul24((uint32_t)cc[u], (uint32_t)row_bytes) + boff));
            else
                xv[slot][u] = *reinterpret_cast<const f4 *>(Xb + (int64_t)cc[u] * row_bytes + boff);
        }
        if (++ii == nst) {  // uniform
            ii = 0;
            ++is;
            col_i = slice_col(min(is, n_slices - 1));
        }
    };
    int fs = 0, fi = 0;  // the FMA cursor: (slice, step)
    // the step's S values come from LDS when its FMAs run (the block is never
    // restaged), read ahead of the next step's gathers: four registers, not
    // four per step in flight
    auto vals = [&]() { return *reinterpret_cast<const f4 *>(&s_val[wl][0][lds_row + fi * U]); };
    auto fma = [&](int slot, const f4 &vq) {
        const int cur = fi * U;
        if (cur + U <= n_min) {  // both rows have these U (uniform)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v)
                    acc[v] = __builtin_fmaf(vq[u], xv[slot][u][v], acc[v]);
        } else {  // a row ends inside this step: per-lane predication
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (cur + u < len) {
#pragma unroll
                    for (int v = 0; v < V; ++v)
                        acc[v] = __builtin_fmaf(vq[u], xv[slot][u][v], acc[v]);
                }
            }
        }
        if (++fi == nst) {  // uniform: the slice is complete
            store(fs, acc);
            fi = 0;
            ++fs;
            if constexpr (ACC)
                acc = accN;
            else
                acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    };
    issue(0);
    if constexpr (ACC) acc = accN;
    for (int t = 0; t < T; t += 2) {  // steps t (slot 0) and t + 1 (slot 1)
        const f4 v0 = vals();
        if (t + 1 < T) issue(1);
        fma(0, v0);
        if (t + 1 >= T) break;
        const f4 v1 = vals();
        if (t + 2 < T) issue(0);
        fma(1, v1);
    }
}

// HF > 0: the fused rows + hub launch (small graphs whose hub chains are
// short, SGC_SPMM_HUB_SERIAL): the first n_hub_blocks workgroups of slice 0
// each run one (hub row, HF-float chunk) item of the hub kernel with three
// loader waves and the chain wave (hub_body<HF, 3>, the rows kernel's 256
// threads), every other workgroup the rows kernel's work -- one launch, so
// the hub chains run beside the light rows with no second launch and no
// cross-stream fork / join (Pubmed shape: the serial hub kernel added its
// whole 15 us chain to every hop).
//
// WD > 0: the launch with wide items (wide_rows_body, LBW = WD; LR = 32, a
// light order, at least two slices).  Its grid is one-dimensional: the
// slice_blocks workgroups of each of the n_slices slices in turn -- the same
// x-fastest sweep as the two-dimensional grid's -- and wide_blocks workgroups
// of wide waves before them (wide_first) or after.  The per-slice light items
// are the n_rows light rows above the wide threshold; light_rows[n_rows ..
// n_rows + n_wide) are the wide rows, and no per-slice wave exists for them.
template <int LB, int VH, int UH, bool O32, int QV, int HF = 0, int WD = 0>
__global__ __launch_bounds__(256) void spmm_rows_kernel(
    const int *__restrict__ row_ptr, const int *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, int64_t ldx, float *__restrict__ Y, int64_t ldy,
    int row_begin, int n_rows, int F, int F_load, int LR, int vec_store, int n_sub,
    const int *__restrict__ heavy_rows, int n_heavy, int heavy_threshold, int accum,
    const int *__restrict__ light_rows, int heavy_pairs, const int *__restrict__ hub_rows = nullptr,
    int hub_chunks = 0, int n_hub_blocks = 0, int n_wide = 0, int wide_blocks = 0,
    int slice_blocks = 0, int n_slices = 0, int wide_first = 0) {
    int bx = (int)blockIdx.x;
    if constexpr (HF > 0) {
        if (bx < n_hub_blocks) {  // block-uniform
            if (blockIdx.y == 0)
                hub_body<HF, 3, kFusedHubInstr>(bx, row_ptr, col, val, X, ldx, Y, ldy, row_begin, F, hub_rows,
                                hub_chunks, accum);
            return;
        }
        bx -= n_hub_blocks;
    }
    constexpr int V = 4, U = kRowsU < LB / 2 ? kRowsU : LB / 2;
    constexpr int kSteps = LB / U;  // steps per LDS block
    static_assert(kSteps >= 2 && kSteps % 2 == 0, "bad block");
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef int i4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) int s_col[kBlock / kWave][2][kWave];
    __shared__ __attribute__((aligned(16))) float s_val[kBlock / kWave][2][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wl = threadIdx.x / kWave;
    int wd_slice = 0;  // WD > 0: this workgroup's slice in the one-dimensional grid
    if constexpr (WD > 0) {
        static_assert(HF == 0 && QV == 0, "wide items: the plain multi-row launch only");
        int wb = -1;  // block-uniform: this workgroup's index among the wide ones, or -1
        if (wide_first) {
            if (bx < wide_blocks) wb = bx;
            bx -= wide_blocks;
        } else if (bx >= slice_blocks * n_slices) {
            wb = bx - slice_blocks * n_slices;
        }
        if (wb >= 0) {
            const int ww = __builtin_amdgcn_readfirstlane(wb * (kBlock / kWave) + wl);
            if (accum)
                wide_rows_body<WD, O32, true>(ww, wl, lane, row_ptr, col, val, X, ldx, Y, ldy,
                                              row_begin, n_wide, F, F_load, vec_store, n_slices,
                                              light_rows + n_rows, s_col, s_val);
            else
                wide_rows_body<WD, O32, false>(ww, wl, lane, row_ptr, col, val, X, ldx, Y, ldy,
                                               row_begin, n_wide, F, F_load, vec_store, n_slices,
                                               light_rows + n_rows, s_col, s_val);
            return;
        }
        wd_slice = bx / slice_blocks;  // (slice_blocks > 0: a per-slice block exists)
        bx -= wd_slice * slice_blocks;
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(bx * (kBlock / kWave) + wl));
    const int slice = WD > 0 ? wd_slice : (int)blockIdx.y;
    const int R = kWave / LR;  // rows per wave (uniform)
    // where this slice's computed columns stop: lanes at or beyond it are idle
    const int seg_end = min(F_load, (slice + 1) * (LR * V));
    const int n_heavy_items = n_heavy * n_sub;
    if (wave < n_heavy_items) {
        const int h = wave / n_sub;
        const int row = heavy_rows[h];
        const int k0 = row_ptr[row], k1 = row_ptr[row + 1];
        if constexpr (QV == 4) {  // 16 lanes x 16 B per nonzero, transposed chains
            const int f = slice * (LR * V) + (lane & 15) * 4;
            row_quadsT_pipe<kQuadsU, O32>(col, val, k0, k1, X, ldx,
                                          Y + (int64_t)(row - row_begin) * ldy, F, f, seg_end,
                                          lane, accum != 0);
            return;
        } else if constexpr (QV > 0) {  // 16 lanes per row: four nonzeros per load
            const int f = slice * (LR * V) + (lane & 15) * QV;
            row_quads_pipe<QV, kQuadsU, O32>(col, val, k0, k1, X, ldx,
                                             Y + (int64_t)(row - row_begin) * ldy, F, f,
                                             seg_end, vec_store != 0, lane, accum != 0);
            return;
        }
        if (heavy_pairs & 1) {  // n_sub == 1: one item per (row, slice), two nonzeros per load
            const int f = slice * (LR * V) + (lane & 31) * V;  // active below seg_end
            if (heavy_pairs & 16)
                row_pairs_pipe<kPairsU, O32, true>(col, val, k0, k1, X, ldx,
                                                   Y + (int64_t)(row - row_begin) * ldy, F, f,
                                                   seg_end, vec_store != 0, lane, accum != 0);
            else
                row_pairs_pipe<kPairsU, O32>(col, val, k0, k1, X, ldx,
                                             Y + (int64_t)(row - row_begin) * ldy, F, f,
                                             seg_end, vec_store != 0, lane, accum != 0);
            return;
        }
        const int sub = slice * n_sub + (wave - h * n_sub);  // in units of 64*VH floats
        if (sub * kWave * VH >= F) return;
        row_chunks_pipe<VH, 1, UH / VH>(col, val, k0, k1, X, ldx,
                                        Y + (int64_t)(row - row_begin) * ldy, F, sub, lane,
                                        accum != 0);
        return;
    }
    const int sub = lane / LR, l = lane - sub * LR;
    int r = 0, k0 = 0, len = 0;
    bool mine = false;
    if (light_rows) {  // light rows in the plan's order (n_rows of them here)
        const int w = wave - n_heavy_items;
        if (w * R >= n_rows) return;  // wave-uniform
        const int li = w * R + sub;
        if (sub < R && li < n_rows) {
            const int row = light_rows[li];
            r = row - row_begin;
            k0 = row_ptr[row];
            len = row_ptr[row + 1] - k0;
            mine = true;
        }
    } else {
        const int w = wave - n_heavy_items;
        if (w * R >= n_rows) return;  // wave-uniform
        r = w * R + sub;
        if (sub < R && r < n_rows) {
            k0 = row_ptr[row_begin + r];
            const int d = row_ptr[row_begin + r + 1] - k0;
            mine = d <= heavy_threshold;  // longer rows: heavy items / hub kernel
            len = mine ? d : 0;
        }
    }
    // the wave runs to its longest row; up to its shortest every step is
    // unpredicated (rows in length order make the two close)
    int n_max = 0, n_min = INT32_MAX, k_max = 0;  // k_max: first nonzero of the longest row
    for (int s = 0; s < R; ++s) {
        const int ls = __builtin_amdgcn_readlane(len, s * LR);
        const int ks = __builtin_amdgcn_readlane(k0, s * LR);
        if (ls > n_max) k_max = ks;
        n_max = max(n_max, ls);
        n_min = min(n_min, ls);
    }
    const int f = slice * (LR * V) + l * V;
    const bool ok = sub < R && f < seg_end;
    // idle lanes (beyond the ragged last slice, or the lanes past the wave's
    // R rows, which alias row 0's lanes) stay on a line an active lane reads
    const uint32_t boff = uint32_t(gather_col(f, seg_end, V)) * 4u;
    const int lds_row = (sub < R ? sub : 0) * LB;  // this lane's row block in LDS
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    // accumulate: continue the chains an earlier column-block pass stored;
    // rows without nonzeros in this pass are neither read nor written
    const bool store = mine && ok && (!accum || len > 0);
    if (accum && store) {
        const float *yr = Y + (int64_t)r * ldy;
        if (vec_store)
            acc = *reinterpret_cast<const f4 *>(yr + f);
        else  // a caller's rows: 4-B aligned, nothing readable from column F on
            acc = load_upto<V>(yr, f, F);
    }
    if (n_max > 0) {
        const char *Xb = reinterpret_cast<const char *>(X);
        const int64_t row_bytes = ldx * 4;
        // lanes l < LB stage (col, val) of their row's nonzero base + l,
        // clamped to its last one; a row without nonzeros stages (and then
        // gathers) what the wave's longest row does (its FMAs are all skipped)
        const bool stager = sub < R && l < LB;
        // Never predicated: a conditional load makes (c, v) a phi whose
        // default copy must wait for every load in flight (s_waitcnt
        // vmcnt(0) once per block: the gathers of the steps ahead drained
        // at every LB nonzeros).  Lanes without a nonzero to stage repeat the
        // address of a lane that has one (stage_index, lane_lines.h): lanes
        // l >= LB their row's lane LB - 1, lanes of an empty row or of no row
        // the longest row's (n_max > 0: it has nonzeros); the value is either
        // not staged or belongs to a row whose FMAs are all skipped.
        const int k0_s = len > 0 ? k0 : k_max, len_s = len > 0 ? len : n_max;
        auto fetch = [&](int base, int &c, float &v) {
            const int kk = k0_s + stage_index(base, l, LB, len_s);
            c = col[kk];
            v = val[kk];
        };
        auto stage = [&](int buf, int c, float v) {
            if (stager) {
                s_col[wl][buf][lds_row + l] = c;
                s_val[wl][buf][lds_row + l] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        int colB;
        float valB;
        {
            int c0;
            float v0;
            fetch(0, c0, v0);
            stage(0, c0, v0);
        }
        fetch(LB, colB, valB);
        f4 xv[2][U];
        float vv[2][U];
        auto issue = [&](int buf, int i, int slot) {
#pragma unroll
            for (int q = 0; q < U / 4; ++q) {
                const i4 cc =
                    *reinterpret_cast<const i4 *>(&s_col[wl][buf][lds_row + i * U + 4 * q]);
                const f4 vq =
                    *reinterpret_cast<const f4 *>(&s_val[wl][buf][lds_row + i * U + 4 * q]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    vv[slot][4 * q + u] = vq[u];
                    if constexpr (O32)  // X spans < 4 GiB: 32-bit row offsets (saddr loads)
                        xv[slot][4 * q + u] = *reinterpret_cast<const f4 *>(
                            Xb + (__umul24((uint32_t)cc[u], (uint32_t)row_bytes) + boff));
                    else
                        xv[slot][4 * q + u] =
                            *reinterpret_cast<const f4 *>(Xb + (int64_t)cc[u] * row_bytes + boff);
                }
            }
        };
        issue(0, 0, 0);
        for (int base = 0;; base += LB) {
            const int buf = (base / LB) & 1;
#pragma unroll
            for (int i = 0; i < kSteps; ++i) {
                const int cur = base + i * U;
                if (cur >= n_max) break;  // wave-uniform
                if (i + 1 < kSteps) {
                    issue(buf, i + 1, (i + 1) & 1);
                } else {  // first step of the next block, from its prefetched (col, val)
                    stage(buf ^ 1, colB, valB);
                    issue(buf ^ 1, 0, 0);
                }
                if (cur + U <= n_min) {  // every row of the wave has these U (uniform)
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int v = 0; v < V; ++v)
                            acc[v] = __builtin_fmaf(vv[i & 1][u], xv[i & 1][u][v], acc[v]);
                } else {  // a row ends inside this step: per-lane predication
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (cur + u < len) {
#pragma unroll
                            for (int v = 0; v < V; ++v)
                                acc[v] = __builtin_fmaf(vv[i & 1][u], xv[i & 1][u][v], acc[v]);
                        }
                    }
                }
            }
            if (base + LB >= n_max) break;
            fetch(base + 2 * LB, colB, valB);
        }
    }
    if (store) {
        float *yr = Y + (int64_t)r * ldy;
        if (vec_store)
            *reinterpret_cast<f4 *>(yr + f) = acc;
        else  // one 16-B store per lane; only the lane that straddles F goes scalar
            store_upto<V>(yr, f, F, acc);
    }
}

template <int HC, int NL>
__global__ __launch_bounds__(64 * (NL + 1)) void spmm_hub_kernel(
    const int *__restrict__ row_ptr, const int *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, int64_t ldx, float *__restrict__ Y, int64_t ldy, int row_begin,
    int F, const int *__restrict__ hub_rows, int n_chunks, int accum) {
    hub_body<HC, NL, kHubInstr>((int)blockIdx.x, row_ptr, col, val, X, ldx, Y, ldy, row_begin, F,
                                hub_rows, n_chunks, accum);
}

namespace {

static_assert(kSchedWavesPerBlock == kBlock / kWave && kSchedWave == kWave,
              "spmm_schedule.h sizes its grids for this workgroup");

struct LaunchArgs {
    const int *row_ptr;
    const int *col;
    const float *val;
    const float *X;
    int64_t ldx;
    float *Y;
    int64_t ldy;
    int row_begin, n_rows, F;
    const int *heavy_rows;  // the light kernel's heavy rows (the hub rows taken off)
    int heavy_threshold;
    int accum;
    hipStream_t stream;
    const int *light_rows;  // SGC_SPMM_LIGHT_ORDER: the light rows in processing order, or null
    const int *hub_rows;    // the hub rows (spmm_hub_kernel, or the fused items of HF = 32)
};

// A side stream + fork/join events per (device, caller's stream) for the
// light kernel of a concurrent launch (the hub kernel stays on the caller's
// stream; the two are ordered against it by events, so the pair is
// capturable into a hipGraph).  One side stream per caller stream, so two
// callers' launches on different streams (the line partition's main and tail
// launches) never queue behind each other on a shared side stream.  The whole fork ->
// launch -> join sequence of one sgc_spmm call runs under `mu`: another host
// thread can neither re-record `fork` between this call's record and wait
// (which would order the hub kernel after the wrong stream) nor enqueue on
// the side stream while a capture holds it.
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    std::mutex mu;
};

// The side streams themselves come from a small per-device pool, created
// once (sgc_warmup creates it, with the loaders): hipStreamCreate took 7.8 ms
// for the process's first side stream (a new hardware queue), inside the first
// sgc_precompute the reference times (profiles/r06/s10: the first Reddit-shape
// call 16.2 ms against 8.2 on a second adjacency).  Caller streams take pool
// streams in turn; past kSidePool callers two callers share one (their light
// kernels then serialise on it: still correct, ordered by their own events).
constexpr int kSidePool = 4;
static std::mutex g_side_mu;

static hipError_t side_pool(int dev, hipStream_t **pool) {
    static std::map<int, std::vector<hipStream_t>> pools;
    std::vector<hipStream_t> &v = pools[dev];
    if (v.empty()) {
        // (a highest-priority side stream measured neutral, +-1%:
        // profiles/r01_hub_priority_sweep.log)
        for (int k = 0; k < kSidePool; ++k) {
            hipStream_t st = nullptr;
            hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e != hipSuccess) return e;
            v.push_back(st);
        }
    }
    *pool = v.data();
    return hipSuccess;
}

hipError_t warm_side_streams_impl() {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_side_mu);
    hipStream_t *pool = nullptr;
    return side_pool(dev, &pool);
}

hipError_t side_stream(SideStream **out, hipStream_t caller) {
    static std::map<std::pair<int, hipStream_t>, SideStream> per_dev;
    static std::map<int, int> next_pool;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_side_mu);
    SideStream &ss = per_dev[{dev, caller}];
    if (!ss.s) {
        hipStream_t *pool = nullptr;
        if ((e = side_pool(dev, &pool)) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming)) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&ss.join, hipEventDisableTiming)) != hipSuccess) return e;
        ss.s = pool[next_pool[dev]++ % kSidePool];
    }
    *out = &ss;
    return hipSuccess;
}

// Launch timing (diagnostics, off by default; bench.py turns it on over its
// timed region): each launch_spmm records timing events around its
// light/heavy kernel and around its hub kernel, each on the stream the kernel
// runs on, so the two kernels' durations are measured separately.
// sgc_timing_collect() waits for and returns them.  Not for use inside a
// graph capture.
struct TimedLaunch {
    hipEvent_t l0 = nullptr, l1 = nullptr, h0 = nullptr, h1 = nullptr;
    int kernel = -1;  // light kernel: 0 spmm_csr_kernel, 1 spmm_rows_kernel, 2 / 3 the same with the hub rows fused, -1 none
    bool serial = false;  // hub kernel ran before the light kernel on the same stream
    bool hub_first = false;  // concurrent: hub kernel on the caller's stream, light on the side
};
static std::mutex g_timing_mu;
static bool g_timing = false;
static std::vector<TimedLaunch> g_timed;
static std::vector<hipEvent_t> g_event_pool;

// Launches recorded but not yet collected are capped: timing left on without
// sgc_timing_collect() stops recording instead of growing without bound.
constexpr size_t kMaxTimed = 1 << 16;

hipError_t pooled_event(hipEvent_t *e) {
    if (!g_event_pool.empty()) {
        *e = g_event_pool.back();
        g_event_pool.pop_back();
        return hipSuccess;
    }
    return hipEventCreate(e);
}

// Error-path guards of launch_spmm (called with g_timing_mu held while a
// TimedLaunch is filled): once the hub fork is recorded, the caller's stream
// is always joined to the side stream, and pooled timing events that never
// reached g_timed go back to the pool.
struct SideJoin {
    SideStream *side = nullptr;
    hipStream_t stream = nullptr;
    ~SideJoin() {
        if (!side) return;
        (void)hipEventRecord(side->join, side->s);
        (void)hipStreamWaitEvent(stream, side->join, 0);
    }
    hipError_t join() {  // the normal path: report the join's own errors
        SideStream *s = side;
        side = nullptr;
        hipError_t e = hipEventRecord(s->join, s->s);
        return e != hipSuccess ? e : hipStreamWaitEvent(stream, s->join, 0);
    }
};

struct TimedGuard {
    TimedLaunch *tl = nullptr;  // non-null while its events are not in g_timed
    ~TimedGuard() {
        if (!tl) return;
        for (hipEvent_t ev : {tl->l0, tl->l1, tl->h0, tl->h1})
            if (ev) g_event_pool.push_back(ev);
    }
    void commit() {
        g_timed.push_back(*tl);
        tl = nullptr;
    }
};

// Nonzeros per step: light items keep U*C*V <= ~40 registers of gathered X
// per step; heavy sub-chunk items go deeper (UH).  The pipelined loop holds
// two steps (measured best at 8 / 16: 48 VGPRs, 8 waves per SIMD, -3% per hop
// vs. an unpipelined U = 16 / 32; profiles/r01_sweep_pipe.log).
constexpr int kHeavyU = 16;

template <int V, int C, int HF = 0>
hipError_t launch_vc(const LaunchArgs &a, const SpmmSchedule &s) {
    constexpr int U0 = (C * V >= 16) ? 2 : (C * V >= 8) ? 4 : 8;
    constexpr int U = U0;
    constexpr int UH = kHeavyU;
    hipLaunchKernelGGL((spmm_csr_kernel<V, C, U, UH, HF>), dim3((unsigned)s.grid_x, (unsigned)s.grid_y),
                       dim3(kBlock), 0, a.stream, a.row_ptr, a.col, a.val, a.X, a.ldx, a.Y, a.ldy,
                       a.row_begin, a.n_rows, s.F_load, a.heavy_rows, s.n_heavy, a.heavy_threshold,
                       a.accum, s.kernel_bits, HF ? a.hub_rows : nullptr, s.fused_chunks,
                       s.fused_blocks);
    return hipGetLastError();
}

template <int V, int C>
hipError_t dispatch_c(const LaunchArgs &a, const SpmmSchedule &s) {
    if constexpr (C == 0) {
        return hipErrorInvalidValue;
    } else {
        if (s.C == C) return launch_vc<V, C>(a, s);
        return dispatch_c<V, C - 1>(a, s);
    }
}

template <int LB, int VH, bool O32, int QV, int HF = 0>
hipError_t launch_rows(const LaunchArgs &a, const SpmmSchedule &s) {
    hipLaunchKernelGGL((spmm_rows_kernel<LB, VH, kHeavyU, O32, QV, HF>),
                       dim3((unsigned)s.grid_x, (unsigned)s.grid_y), dim3(kBlock), 0, a.stream,
                       a.row_ptr, a.col, a.val, a.X, a.ldx, a.Y, a.ldy, a.row_begin,
                       s.n_light_items, a.F, s.F_load, s.LR, s.vec_store, s.n_sub, a.heavy_rows,
                       s.n_heavy, a.heavy_threshold, a.accum, a.light_rows, s.kernel_bits,
                       HF ? a.hub_rows : nullptr, s.fused_chunks, s.fused_blocks);
    return hipGetLastError();
}

// The launch with wide items (spmm_rows_kernel WD > 0; LR = 32, a light
// order, at least two slices): a one-dimensional grid (spmm_schedule).
template <int VH, bool O32, int WD>
hipError_t launch_rows_wide(const LaunchArgs &a, const SpmmSchedule &s) {
    hipLaunchKernelGGL((spmm_rows_kernel<16, VH, kHeavyU, O32, 0, 0, WD>), dim3((unsigned)s.grid_x),
                       dim3(kBlock), 0, a.stream, a.row_ptr, a.col, a.val, a.X, a.ldx, a.Y, a.ldy,
                       a.row_begin, s.n_light_items, a.F, s.F_load, s.LR, s.vec_store, s.n_sub,
                       a.heavy_rows, s.n_heavy, a.heavy_threshold, a.accum, a.light_rows,
                       s.kernel_bits, nullptr, 0, 0, s.n_wide, (int)s.wide_blocks,
                       (int)s.slice_blocks, s.slices, s.wide_first);
    return hipGetLastError();
}

}  // namespace

// The concurrent hub launch's fork / join for the 16-bit-feature launches
// (spmm16.hip), on the same per-caller-stream side streams as launch_spmm:
// *light = the side stream, ordered after `stream`'s work so far; the side
// stream's mutex stays held until join_light_stream(*side, stream), which
// makes `stream` wait for the side stream.  Every successful fork is joined.
int fork_light_stream(hipStream_t stream, hipStream_t *light, void **side_out) {
    SideStream *side = nullptr;
    SGC_HIP_CHECK(side_stream(&side, stream));
    side->mu.lock();
    hipError_t e = hipEventRecord(side->fork, stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(side->s, side->fork, 0);
    if (e != hipSuccess) {
        side->mu.unlock();
        set_error("spmm: side-stream fork failed: %s", hipGetErrorString(e));
        return SGC_EHIP;
    }
    *light = side->s;
    *side_out = side;
    return SGC_OK;
}

int join_light_stream(void *side_in, hipStream_t stream) {
    SideStream *side = static_cast<SideStream *>(side_in);
    hipError_t e = hipEventRecord(side->join, side->s);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, side->join, 0);
    side->mu.unlock();
    SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "spmm: side-stream join failed: %s",
                hipGetErrorString(e));
    return SGC_OK;
}

// The SpMM knobs (spmm_schedule.h describes each) and the knob table: one
// row per sgc_set_tuning key -- where it lives, what it accepts, what a
// rejected value is told.  get_tuning reads the same rows.
static SpmmKnobs g_knobs;
// launches that took wide items since the library was loaded (diagnostics)
static std::atomic<int64_t> g_short_wide_launches{0};

namespace {
struct Knob {
    const char *name;
    int *value;
    bool (*ok)(int64_t);
    const char *message;
};
template <int64_t... Vs>
bool one_of(int64_t v) { return ((v == Vs) || ...); }
template <int64_t Lo, int64_t Hi>
bool within(int64_t v) { return v >= Lo && v <= Hi; }
const Knob kKnobs[] = {
    {"slice_floats", &g_knobs.slice_floats, within<0, (1 << 20) - 1>, "slice_floats out of range"},
    {"hub_chunk", &g_knobs.hub_chunk, one_of<0, 32, 64>, "hub_chunk must be 0 (auto), 32 or 64"},
    {"hub_loaders", &g_knobs.hub_loaders, one_of<7, 15>, "hub_loaders must be 7 or 15"},
    {"hub_fuse", &g_knobs.hub_fuse, one_of<0, 1>, "hub_fuse must be 0 or 1"},
    {"hub_stream", &g_knobs.hub_stream, within<0, 2>, "hub_stream must be 0, 1 or 2"},
    {"rows_per_wave", &g_knobs.rows_per_wave, one_of<0, 1, 2, 4>,
     "rows_per_wave must be 0 (auto), 1, 2 or 4"},
    {"heavy_pairs", &g_knobs.heavy_pairs, within<0, 31>, "heavy_pairs must be 0..31 (a bit mask)"},
    {"x16_vec", &g_x16_vec, one_of<0, 1, 2, 4, 8>, "x16_vec must be 0 (auto), 1, 2, 4 or 8"},
    {"x16_step", &g_x16_step, one_of<0, 4, 8>, "x16_step must be 0 (auto), 4 or 8"},
    {"tile_buffers", &g_tile_buffers, one_of<1, 2>, "tile_buffers must be 1 or 2"},
    {"linear_ck", &g_linear_ck, one_of<32, 64>, "linear_ck must be 32 or 64"},
    {"linear_kernel", &g_linear_kernel, within<0, 8>, "linear_kernel must be 0..8"},
    {"backward_kernel", &g_backward_kernel, within<0, 3>, "backward_kernel must be 0..3"},
    {"max_vec", &g_knobs.max_vec, one_of<1, 2, 4>, "max_vec must be 1, 2 or 4"},
    {"short_wide", &g_knobs.short_wide, within<-1, 32>,
     "short_wide must be -1 (the rule), 0 (off) or 1..32"},
    {"short_wide_first", &g_knobs.short_wide_first, one_of<0, 1>, "short_wide_first must be 0 or 1"},
};
}  // namespace

int set_tuning(const char *key, int64_t value) {
    SGC_REQUIRE(key, SGC_EINVAL, "set_tuning: null key");
    for (const Knob &k : kKnobs) {
        if (std::strcmp(key, k.name) != 0) continue;
        SGC_REQUIRE(k.ok(value), SGC_EINVAL, "%s", k.message);
        *k.value = (int)value;
        return SGC_OK;
    }
    set_error("set_tuning: unknown key '%s'", key);
    return SGC_EINVAL;
}

int64_t get_tuning(const char *key) {
    if (!key) return -1;
    const int sw = g_knobs.short_wide;
    // (first: the Python layer reads it once per propagate() call)
    if (std::strcmp(key, "short_wide_state") == 0)
        return (int64_t)(sw + 1) * 64 + (sw < 0 ? kShortWideTs : sw);
    for (const Knob &k : kKnobs)
        if (std::strcmp(key, k.name) == 0) return *k.value;
    if (std::strcmp(key, "short_wide_ts") == 0) return sw < 0 ? kShortWideTs : sw;
    if (std::strcmp(key, "short_wide_launches") == 0) return g_short_wide_launches.load();
    return -1;
}

namespace {

// The shape spmm_schedule looks at, from a call whose arguments passed
// `validate` (the checks launch_spmm makes before anything else); *empty: a
// launch over no rows, or SGC_SPMM_HUB_ONLY without hub rows -- nothing to do.
int spmm_shape(const SpmmCall &c, bool validate, SpmmShape *sh, bool *empty) {
    if (validate) {
        // col_idx / val may be NULL for a CSR without nonzeros (torch's empty
        // tensors have no storage): the kernels never dereference them then
        SGC_REQUIRE(c.row_ptr && c.X && c.Y, SGC_EINVAL, "spmm: null pointer");
    }
    SGC_REQUIRE(c.row_begin >= 0 && c.row_end >= c.row_begin && c.row_end < INT32_MAX, SGC_ERANGE,
                "spmm: bad row range [%lld, %lld)", (long long)c.row_begin, (long long)c.row_end);
    SGC_REQUIRE(c.F > 0 && c.F < (1 << 24), SGC_EINVAL, "spmm: bad feature count %lld",
                (long long)c.F);
    SGC_REQUIRE(c.ldx >= c.F && c.ldy >= c.F, SGC_EINVAL, "spmm: ldx/ldy (%lld/%lld) < F (%lld)",
                (long long)c.ldx, (long long)c.ldy, (long long)c.F);
    SGC_REQUIRE(c.n_heavy >= 0 && (c.n_heavy == 0 || c.plan), SGC_EINVAL, "spmm: bad plan");
    sh->n_rows = c.row_end - c.row_begin;
    *empty = sh->n_rows == 0;
    if (*empty) return SGC_OK;
    char err[160];
    const int rc = spmm_plan_prologue("spmm", sh->n_rows, c.plan != nullptr, c.n_heavy, c.n_hub,
                                      c.heavy_threshold, c.flags, c.n_nonempty, c.n_not_wide,
                                      c.wide_max_nnz, g_knobs.short_wide, &sh->plan, err,
                                      sizeof(err));
    SGC_REQUIRE(rc == SGC_OK, rc, "%s", err);
    *empty = (c.flags & SGC_SPMM_HUB_ONLY) && sh->plan.n_hub == 0;
    sh->F = c.F;
    sh->ldx = c.ldx;
    sh->ldy = c.ldy;
    sh->x_addr = reinterpret_cast<uintptr_t>(c.X);
    sh->y_addr = reinterpret_cast<uintptr_t>(c.Y);
    sh->flags = c.flags;
    sh->wide_max_nnz = c.wide_max_nnz;
    return SGC_OK;
}

hipError_t launch_hub(const LaunchArgs &a, const SpmmSchedule &s) {
#define SGC_LAUNCH_HUB(HCV, NLV)                                                                \
    hipLaunchKernelGGL((spmm_hub_kernel<HCV, NLV>), dim3((unsigned)s.hub_grid),                 \
                       dim3(64 * (NLV + 1)), 0, a.stream, a.row_ptr, a.col, a.val, a.X, a.ldx,  \
                       a.Y, a.ldy, a.row_begin, a.F, a.hub_rows, s.hub_n_chunks, a.accum)
    if (s.hub_chunk == 32) {
        if (s.hub_loaders == 7) SGC_LAUNCH_HUB(32, 7);
        else SGC_LAUNCH_HUB(32, 15);
    } else {
        if (s.hub_loaders == 7) SGC_LAUNCH_HUB(64, 7);
        else SGC_LAUNCH_HUB(64, 15);
    }
#undef SGC_LAUNCH_HUB
    return hipGetLastError();
}

// The schedule's light kernel: one line per template instantiation.
hipError_t launch_light(const LaunchArgs &a, const SpmmSchedule &s) {
    if (s.grid_x == 0) return hipSuccess;  // an accumulate launch over empty runs
    if (s.multi_row && s.WD) {
#define SGC_WIDE(VHV, WDV)                                                  \
    if (s.VH == VHV && s.WD == WDV)                                         \
        return s.O32 ? launch_rows_wide<VHV, true, WDV>(a, s)               \
                     : launch_rows_wide<VHV, false, WDV>(a, s)
        SGC_WIDE(2, 16);
        SGC_WIDE(1, 16);
        SGC_WIDE(2, 32);
        SGC_WIDE(1, 32);
#undef SGC_WIDE
    } else if (s.multi_row) {
#define SGC_ROWS(LBV, VHV, QVV, HFV)                                        \
    if (s.LB == LBV && s.VH == VHV && s.QV == QVV && s.HF == HFV)           \
        return s.O32 ? launch_rows<LBV, VHV, true, QVV, HFV>(a, s)          \
                     : launch_rows<LBV, VHV, false, QVV, HFV>(a, s)
        SGC_ROWS(16, 2, 4, 0);
        SGC_ROWS(8, 2, 4, 0);
        SGC_ROWS(8, 2, 2, 0);
        SGC_ROWS(8, 2, 1, 0);
        SGC_ROWS(16, 2, 0, 32);
        SGC_ROWS(16, 2, 0, 0);
        SGC_ROWS(16, 1, 0, 0);
        SGC_ROWS(8, 2, 0, 0);
        SGC_ROWS(8, 1, 0, 0);
#undef SGC_ROWS
    } else if (s.HF) {
        return launch_vc<4, 1, 32>(a, s);
    } else if (s.V == 4) {
        return dispatch_c<4, 16 / 4>(a, s);  // <= 16 accumulators per lane
    } else if (s.V == 2) {
        return dispatch_c<2, 16 / 2>(a, s);
    } else {
        return dispatch_c<1, 16 / 1>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// validate -> prologue -> spmm_schedule (spmm_schedule.h: every choice) ->
// side stream and timing -> the schedule's launches.
int launch_spmm(const SpmmCall &c, hipStream_t stream) {
    SpmmShape sh;
    bool empty = false;
    int rc = spmm_shape(c, true, &sh, &empty);
    if (rc != SGC_OK || empty) return rc;
    SpmmSchedule s;
    char err[160];
    rc = spmm_schedule(sh, g_knobs, &s, err, sizeof(err));
    SGC_REQUIRE(rc == SGC_OK, rc, "%s", err);

    SideStream *side = nullptr;
    std::unique_lock<std::mutex> side_lock;
    std::unique_lock<std::mutex> timing_lock(g_timing_mu);
    TimedLaunch tl;
    const bool timing = g_timing && g_timed.size() < kMaxTimed;
    if (!timing) timing_lock.unlock();
    // declared after the locks: destroyed (join, events back to the pool)
    // while they are still held
    TimedGuard timed_guard;
    if (timing) timed_guard.tl = &tl;
    SideJoin side_join;
    const int32_t *hub_rows = c.plan ? c.plan + sh.plan.heavy_skip : nullptr;
    LaunchArgs a{c.row_ptr, c.col_idx, c.val, c.X, c.ldx, c.Y, c.ldy, (int)c.row_begin,
                 (int)sh.n_rows, (int)c.F, hub_rows ? hub_rows + sh.plan.n_hub : nullptr,
                 sh.plan.heavy_threshold, (c.flags & SGC_SPMM_ACCUMULATE) ? 1 : 0, stream,
                 // (used by the multi-row kernel; the one-row kernel: natural order)
                 sh.plan.light_offset >= 0 ? c.plan + sh.plan.light_offset : nullptr, hub_rows};
    if (s.hub == kHubConcurrent) {
        SGC_HIP_CHECK(side_stream(&side, stream));
        side_lock = std::unique_lock<std::mutex>(side->mu);
        SGC_HIP_CHECK(hipEventRecord(side->fork, stream));
        SGC_HIP_CHECK(hipStreamWaitEvent(side->s, side->fork, 0));
        side_join.side = side;  // from here on every exit joins
        side_join.stream = stream;
        tl.hub_first = true;
    }
    if (s.hub == kHubConcurrent || s.hub == kHubSerial) {
        // the hub kernel: always on the caller's stream
        if (timing) {
            SGC_HIP_CHECK(pooled_event(&tl.h0));
            SGC_HIP_CHECK(pooled_event(&tl.h1));
            SGC_HIP_CHECK(hipEventRecord(tl.h0, stream));
            tl.serial = s.hub == kHubSerial;
        }
        SGC_HIP_CHECK(launch_hub(a, s));
        if (timing) SGC_HIP_CHECK(hipEventRecord(tl.h1, stream));
    }
    if (side) a.stream = side->s;  // the light kernel beside the hub kernel
    if (timing) {  // (SGC_SPMM_HUB_ONLY: no light kernel, an empty light interval)
        SGC_HIP_CHECK(pooled_event(&tl.l0));
        SGC_HIP_CHECK(pooled_event(&tl.l1));
        SGC_HIP_CHECK(hipEventRecord(tl.l0, a.stream));
        tl.kernel = s.kernel;
    }
    if (s.kernel >= 0) {
        if (s.WD) g_short_wide_launches.fetch_add(1, std::memory_order_relaxed);
        const hipError_t e = launch_light(a, s);
        SGC_REQUIRE(e == hipSuccess, SGC_EHIP, "spmm launch failed: %s", hipGetErrorString(e));
    }
    if (timing) {
        SGC_HIP_CHECK(hipEventRecord(tl.l1, a.stream));
        timed_guard.commit();
    }
    if (side) SGC_HIP_CHECK(side_join.join());  // the caller's stream waits for the hub kernel
    return SGC_OK;
}

const char *spmm_kernel_name(const SpmmCall &c) {
    static thread_local char name[256];
    SpmmShape sh;
    SpmmSchedule s;
    bool empty = false;
    char err[160];
    if (spmm_shape(c, false, &sh, &empty) != SGC_OK) return "none";
    if (empty) return "none";
    if (spmm_schedule(sh, g_knobs, &s, err, sizeof(err)) != SGC_OK) {
        set_error("%s", err);
        return "none";
    }
    spmm_schedule_name(s, name, sizeof(name));
    return name;
}

#if SGC_HUB_STAMPS
extern "C" int sgc_debug_hub_stamps(unsigned long long *host, int64_t n) {
    const int64_t cap = 5 * (int64_t)kStampRounds;
    SGC_HIP_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_hub_stamp),
                                      sizeof(unsigned long long) * (n < cap ? n : cap)));
    return SGC_OK;
}
#endif

int timing_enable(int on) {
    std::lock_guard<std::mutex> lock(g_timing_mu);
    g_timing = on != 0;
    return SGC_OK;
}

int timing_collect_ex(float *light_ms, float *hub_ms, float *span_ms, int32_t *kernel,
                      int64_t capacity, int64_t *n_host) {
    SGC_REQUIRE(n_host, SGC_EINVAL, "timing_collect: null n_host");
    std::lock_guard<std::mutex> lock(g_timing_mu);
    const int64_t n = (int64_t)g_timed.size();
    *n_host = n;
    SGC_REQUIRE(capacity >= n && (n == 0 || (light_ms && hub_ms)), SGC_ENOMEM,
                "timing_collect: capacity %lld < %lld launches", (long long)capacity,
                (long long)n);
    for (int64_t i = 0; i < n; ++i) {
        TimedLaunch &t = g_timed[(size_t)i];
        SGC_HIP_CHECK(hipEventSynchronize(t.l1));
        SGC_HIP_CHECK(hipEventElapsedTime(&light_ms[i], t.l0, t.l1));
        hub_ms[i] = -1.0f;
        float span = light_ms[i];
        if (t.h0) {
            SGC_HIP_CHECK(hipEventSynchronize(t.h1));
            SGC_HIP_CHECK(hipEventElapsedTime(&hub_ms[i], t.h0, t.h1));
            float to_end = 0.0f;
            if (t.serial) {  // h0 ... h1 l0 ... l1 on one stream
                SGC_HIP_CHECK(hipEventElapsedTime(&span, t.h0, t.l1));
            } else if (t.hub_first) {  // h0 on the caller's stream, l0 after the fork
                SGC_HIP_CHECK(hipEventElapsedTime(&to_end, t.h0, t.l1));
                span = std::max(hub_ms[i], to_end);
            }
        }
        if (span_ms) span_ms[i] = span;
        if (kernel) kernel[i] = t.kernel;
        for (hipEvent_t ev : {t.l0, t.l1, t.h0, t.h1})
            if (ev) g_event_pool.push_back(ev);
    }
    g_timed.clear();
    return SGC_OK;
}

int timing_collect(float *light_ms, float *hub_ms, int64_t capacity, int64_t *n_host) {
    return timing_collect_ex(light_ms, hub_ms, nullptr, nullptr, capacity, n_host);
}

// ---------------------------------------------------------------------------
// Row re-layout dst[i, 0:F] = src[i, 0:F]: one wave per row, V-float vectors
// (the runtime's 2-D copy blit reached only ~3 TB/s on this shape).
template <int V>
__global__ __launch_bounds__(256) void pad_rows_kernel(const float *__restrict__ src, int64_t lds,
                                                      float *__restrict__ dst, int64_t ldd,
                                                      int64_t n_rows, int F) {
    using VT = typename Vec<V>::T;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x / kWave);
    for (int64_t r = blockIdx.x * (int64_t)(blockDim.x / kWave) + threadIdx.x / kWave; r < n_rows;
         r += waves) {
        const VT *s = reinterpret_cast<const VT *>(src + r * lds);
        VT *d = reinterpret_cast<VT *>(dst + r * ldd);
        for (int i = lane; i < F / V; i += kWave) d[i] = s[i];
    }
}

// (16-B lanes for 8-B aligned source rows -- unaligned dwordx4 loads, aligned
// stores, a scalar tail -- measured no faster than V = 2 at Reddit shape:
// 0.207 vs 0.205 ms, profiles/ragged_lines.)
int launch_pad_rows(const float *src, int64_t lds, float *dst, int64_t ldd, int64_t n_rows,
                    int64_t F, hipStream_t stream) {
    SGC_REQUIRE(src && dst && lds >= F && ldd >= F && n_rows >= 0 && F >= 0 && F < INT32_MAX,
                SGC_EINVAL, "pad_rows: bad arguments");
    if (n_rows == 0 || F == 0) return SGC_OK;
    const int64_t blocks = std::min<int64_t>((n_rows + 3) / 4, 256 * 16);
    const int V = spmm_pick_vec(g_knobs, F, lds, ldd, reinterpret_cast<uintptr_t>(src),
                                reinterpret_cast<uintptr_t>(dst));
    if (V == 4)
        hipLaunchKernelGGL(pad_rows_kernel<4>, dim3(blocks), dim3(256), 0, stream, src, lds, dst,
                           ldd, n_rows, (int)F);
    else if (V == 2)
        hipLaunchKernelGGL(pad_rows_kernel<2>, dim3(blocks), dim3(256), 0, stream, src, lds, dst,
                           ldd, n_rows, (int)F);
    else
        hipLaunchKernelGGL(pad_rows_kernel<1>, dim3(blocks), dim3(256), 0, stream, src, lds, dst,
                           ldd, n_rows, (int)F);
    SGC_HIP_CHECK(hipGetLastError());
    return SGC_OK;
}

// ---------------------------------------------------------------------------
// Plan: list the rows with > threshold nonzeros, heaviest first.
__global__ void heavy_rows_kernel(const int *__restrict__ row_ptr, int row_begin, int n_rows,
                                  int threshold, int *__restrict__ out_pairs,
                                  int *__restrict__ count) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_rows;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int row = row_begin + (int)i;
        const int d = row_ptr[row + 1] - row_ptr[row];
        if (d > threshold) {
            const int pos = atomicAdd(count, 1);
            out_pairs[2 * pos] = d;
            out_pairs[2 * pos + 1] = row;
        }
    }
}

int build_plan(const int32_t *row_ptr, int64_t row_begin, int64_t row_end,
               int32_t threshold, int32_t hub_threshold, int32_t *plan, int64_t capacity,
               int64_t *n_heavy_host, int64_t *n_hub_host, hipStream_t stream) {
    SGC_REQUIRE(row_ptr && plan && n_heavy_host, SGC_EINVAL, "plan: null pointer");
    SGC_REQUIRE(hub_threshold >= threshold, SGC_EINVAL, "plan: hub_threshold < heavy_threshold");
    if (n_hub_host) *n_hub_host = 0;
    const int64_t n_rows = row_end - row_begin;
    SGC_REQUIRE(n_rows >= 0 && row_end < INT32_MAX, SGC_ERANGE, "plan: bad row range");
    SGC_REQUIRE(capacity >= 2 * n_rows + 1, SGC_ENOMEM, "plan: capacity %lld < %lld",
                (long long)capacity, (long long)(2 * n_rows + 1));
    *n_heavy_host = 0;
    if (n_rows == 0) return SGC_OK;
    int *count = plan + 2 * n_rows;  // last word is the counter
    SGC_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int), stream));
    const int blocks = (int)std::min<int64_t>((n_rows + 255) / 256, 4096);
    hipLaunchKernelGGL(heavy_rows_kernel, dim3(blocks), dim3(256), 0, stream, row_ptr,
                       (int)row_begin, (int)n_rows, threshold, plan, count);
    SGC_HIP_CHECK(hipGetLastError());
    int h = 0;
    SGC_HIP_CHECK(hipMemcpyAsync(&h, count, sizeof(int), hipMemcpyDeviceToHost, stream));
    SGC_HIP_CHECK(hipStreamSynchronize(stream));
    if (h > 0) {
        std::vector<int> pairs(2 * (size_t)h);
        SGC_HIP_CHECK(hipMemcpyAsync(pairs.data(), plan, pairs.size() * sizeof(int),
                                     hipMemcpyDeviceToHost, stream));
        SGC_HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<std::pair<int, int>> dr(h);
        for (int i = 0; i < h; ++i) dr[i] = {-pairs[2 * i], pairs[2 * i + 1]};
        std::sort(dr.begin(), dr.end());  // degree desc, then row asc
        std::vector<int> rows(h);
        int64_t hubs = 0;
        for (int i = 0; i < h; ++i) {
            rows[i] = dr[i].second;
            hubs += (-dr[i].first > hub_threshold);
        }
        if (n_hub_host) *n_hub_host = hubs;
        SGC_HIP_CHECK(hipMemcpyAsync(plan, rows.data(), h * sizeof(int), hipMemcpyHostToDevice,
                                     stream));
        SGC_HIP_CHECK(hipStreamSynchronize(stream));
    }
    *n_heavy_host = h;
    return SGC_OK;
}

// Light rows (degree <= threshold) longest first, ties in row order: a
// stable counting sort over the degrees on the host (one read-back of the
// range's row_ptr through a pinned buffer; ~1 ms at Reddit shape).
int light_order(const int32_t *row_ptr, int64_t row_begin, int64_t row_end, int32_t threshold,
                int32_t *light, int64_t *n_light_host, hipStream_t stream) {
    SGC_REQUIRE(row_ptr && light && n_light_host, SGC_EINVAL, "light_order: null pointer");
    const int64_t n_rows = row_end - row_begin;
    SGC_REQUIRE(n_rows >= 0 && row_end < INT32_MAX && threshold >= 0, SGC_ERANGE,
                "light_order: bad row range or threshold");
    *n_light_host = 0;
    if (n_rows == 0) return SGC_OK;
    // pinned staging, kept for the process (grown on demand): a first large
    // pageable device-to-host copy costs the runtime tens of ms
    static std::mutex mu;
    static int32_t *pinned = nullptr;
    static size_t pinned_words = 0;
    std::lock_guard<std::mutex> lock(mu);
    const size_t need = 2 * ((size_t)n_rows + 1);  // row_ptr in, order out
    if (pinned_words < need) {
        if (pinned) SGC_HIP_CHECK(hipHostFree(pinned));
        pinned = nullptr;
        pinned_words = 0;
        SGC_HIP_CHECK(hipHostMalloc((void **)&pinned, need * sizeof(int32_t), hipHostMallocDefault));
        pinned_words = need;
    }
    int32_t *rp = pinned;
    SGC_HIP_CHECK(hipMemcpyAsync(rp, row_ptr + row_begin, ((size_t)n_rows + 1) * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, stream));
    SGC_HIP_CHECK(hipStreamSynchronize(stream));
    // buckets up to the longest light row, not the threshold (which may be
    // huge: "no heavy rows")
    int64_t top = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t d = (int64_t)rp[i + 1] - rp[i];
        if (d <= threshold && d > top) top = d;
    }
    std::vector<int64_t> start((size_t)top + 2, 0);  // bucket t = top - degree
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t d = (int64_t)rp[i + 1] - rp[i];
        if (d <= threshold) ++start[(size_t)(top - d) + 1];
    }
    for (size_t t = 1; t < start.size(); ++t) start[t] += start[t - 1];
    const int64_t n_light = start.back();
    int32_t *out = pinned + n_rows + 1;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t d = (int64_t)rp[i + 1] - rp[i];
        if (d <= threshold) out[(size_t)start[(size_t)(top - d)]++] = (int32_t)(row_begin + i);
    }
    if (n_light > 0) {
        SGC_HIP_CHECK(hipMemcpyAsync(light, out, (size_t)n_light * sizeof(int32_t),
                                     hipMemcpyHostToDevice, stream));
        SGC_HIP_CHECK(hipStreamSynchronize(stream));
    }
    *n_light_host = n_light;
    return SGC_OK;
}

SGC_WARM_UNIT(warm_spmm)

hipError_t warm_side_streams() { return warm_side_streams_impl(); }

}  // namespace sgc
