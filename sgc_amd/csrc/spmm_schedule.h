// spmm_schedule.h -- which kernel, template instantiation and grid an fp32 SpMM
// launch takes, as a pure function of the launch's shape and the tuning knobs.
// Plain C++17 without HIP headers (as lane_lines.h): launch_spmm (spmm.hip)
// launches what spmm_schedule() returns, sgc_spmm_kernel_name reports it, and
// tests/spmm_schedule_host.cpp asserts it with a host compiler.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "sgc_amd.h"

namespace sgc {

constexpr int kSchedWave = 64;          // lanes per wavefront
constexpr int kSchedWavesPerBlock = 4;  // 256-thread light / heavy workgroups

// The SpMM knobs (sgc_set_tuning); each is described where spmm_schedule reads it.
struct SpmmKnobs {
    // Feature-slice width in floats (rounded down to whole 64V-float chunks,
    // at least one).  Default 128: one chunk per slice, so the chip's pass over
    // S touches only X[:, slice] -- 119 MB at the Reddit shape, resident in the
    // 256 MB MALL -- at the price of re-reading the CSR once per slice (8 B/nnz).
    // Measured 4.74 ms/hop at the Reddit shape vs 5.48 ms for 256 and 6.24 ms
    // for 0 = one slice as wide as the registers allow (2.9 GB live X)
    // (profiles/r01_sweep_slices.log).
    int slice_floats = 128;
    int max_vec = 4;  // widest per-lane register vector of the one-row kernel: 1, 2 or 4
    // Light kernel choice when 16-B lanes are possible (F rounded up to 4 fits
    // the rows and they are 16-B aligned): 0 = auto -- spmm_rows_kernel when
    // spmm_csr_kernel could not use 16-B lanes itself (F % 4 != 0: Reddit's 602)
    // or the launch is narrower than 128 floats or a large one at 128 / > 256
    // floats (kWideRowsMin below), else spmm_csr_kernel (F = 152 .. 256, and
    // Pubmed's 500: its one-row 256-float slices measured faster); 2 / 4 = always
    // spmm_rows_kernel with 32 / 16 lanes per row on wide launches; 1 = never.
    // profiles/r02/sweep_rows*.
    int rows_per_wave = 0;
    // Heavy rows, two nonzeros per load instruction (row_pairs_pipe, 16-B lanes)
    // instead of one wave per 64*VH-float sub-chunk (row_chunks_pipe): bit 0 = in
    // the multi-row kernel (Reddit shape K=2: 9.29 -> 9.12 ms, profiles/r03/s1/ab.log),
    // bit 1 = in the one-row kernel; bit 2 = four nonzeros per load instead of two
    // in the multi-row kernel on launches of <= 32 floats (row_quads_pipe); bit 3
    // = the same on 33..64-float launches, transposed (row_quadsT_pipe: one
    // 64-float hop over all Reddit-shape rows 0.715 -> 0.539 ms); bit 4 = the
    // pairs transposed (row_pairs_pipe TR: 76 floats 0.775 -> 0.747 ms, 304
    // floats 2.26 -> 2.16, Reddit K=2 8.11 -> 8.00; profiles/r04/quadsT_ab.log,
    // pairsT_ab.log; all bit-identical).
    int heavy_pairs = 29;
    int hub_chunk = 0;  // hub-kernel feature chunk: 0 = auto (32 on 128-B aligned X rows, else 64)
    // Where the hub kernel runs: 1 = concurrent with the light kernel -- the hub
    // kernel on the caller's stream, the light kernel on a side stream (fork +
    // join events: ~20-30 us of cross-queue synchronisation per launch); 2 = the
    // caller's stream, before the light kernel (serial: costs the hub kernel's
    // own time); 0 = per launch, serial when the caller sets SGC_SPMM_HUB_SERIAL
    // (the Python layer does when the longest hub chain is shorter than that
    // synchronisation: Pubmed shape 70 -> 61 us per hop), else concurrent.
    // Concurrent launches put the HUB kernel on the caller's stream because the
    // stream that waits on the fork event starts a few microseconds later: with
    // the light kernel first, its 256-thread workgroups fill every CU and the
    // 1024-thread hub workgroups trickled in as whole CUs drained, ending up to
    // 0.26 ms after it (profiles/r03/s6 trace); hub first: Reddit K=2 8.96 ->
    // 8.91 ms, one 76-float pass 0.91 -> 0.77 ms (profiles/r03/s7/stream3*.log).
    int hub_stream = 0;
    int hub_loaders = 15;  // loader waves per hub workgroup: 15 or 7 (spmm_hub_kernel)
    // Serial hub rows (SGC_SPMM_HUB_SERIAL) inside the multi-row kernel's launch
    // (spmm_rows_kernel / spmm_csr_kernel HF = 32) instead of a hub kernel launch
    // before it: 1 = on where the launch takes the multi-row kernel over whole
    // 16-B-lane slices or the one-chunk csr kernel.
    int hub_fuse = 1;
    // Wide items (wide_rows_body): light rows of at most Ts nonzeros cross every
    // feature slice in one wave instead of one wave per slice.  0 = off; -1 = the
    // rule (Ts = kShortWideTs on launches of at least kWideRowsMin rows); 1..32
    // forces Ts on every launch that can take them (the multi-row kernel at 32
    // lanes per row, a light order, at least two slices, no fused hub rows).  The
    // caller passes the count of light rows above Ts with Ts itself (the plan
    // counts them for 4 / 8 / 16 / 32), so the knob moves without re-planning;
    // "short_wide_ts" reports the Ts in force (0 = off).
    int short_wide = -1;
    int short_wide_first = 0;  // the wide waves' workgroups before (1) or after (0) the slices' in the grid
};
constexpr int kShortWideTs = 16;

// Large launches with 16-B lanes at F4 == 128 or F4 > 256 take the
// multi-row kernel (128-float slices, two rows per wave) even when
// spmm_csr_kernel could use 16-B lanes: one hop over the Reddit-shape graph
// (interleaved, bit-identical, profiles/r03/s10/ab_reddit.log) at 304 floats
// (the P = 2 feature block) 3.00 -> 2.50 ms, at 128 1.00 -> 0.94; at 152 / 160
// the one-row kernel's single 256-float slice stays faster (1.46 vs 1.60), and
// at 256 it is the RMAT shape's kernel (31.6 vs 37.3 ms per hop).  Small
// launches (Pubmed shape, F = 500) stay latency-bound on the one-row kernel.
constexpr int64_t kWideRowsMin = 65536;
// One-row kernel: row_chunks_pipe2 (whole-block schedule) on launches of at
// least this many rows, row_chunks_pipe below.  Measured bit-identical,
// interleaved (profiles/r03/s5/chunks_*.log): RMAT shape K=3 (4.2 M rows)
// 95.5 -> 94.1 ms; Pubmed shape K=2 (19.7 k rows, latency-bound) 0.102 ->
// 0.109 ms.
constexpr int kChunksPipe2Rows = 1 << 20;

// The plan as the launch uses it (spmm_plan_prologue), in entries of the
// caller's plan array [heavy rows, hub rows first | light rows in order].
struct SpmmPlan {
    bool has_plan = false;
    int64_t heavy_skip = 0;     // plan entries before the first heavy row (SGC_SPMM_NO_HUB: the hub rows)
    int64_t n_heavy = 0;        // heavy rows from there, the n_hub hub rows first
    int64_t n_hub = 0;
    int32_t heavy_threshold = INT32_MAX;
    int64_t light_offset = -1;  // SGC_SPMM_LIGHT_ORDER: the first light row's plan entry, else -1
    int64_t n_light = 0;        // light items of that order (an accumulate launch: those with nonzeros)
    int64_t n_wide = 0;         // the last n_wide of them may run as wide items
};

// The plan prologue of launch_spmm and launch_spmm_x16 (`who` prefixes the
// messages; the 16-bit launch passes n_nonempty = n_not_wide = -1).  Returns
// SGC_OK, or the error code with its text in err.
inline int spmm_plan_prologue(const char *who, int64_t n_rows, bool has_plan, int64_t n_heavy,
                              int64_t n_hub, int32_t heavy_threshold, uint32_t flags,
                              int64_t n_nonempty, int64_t n_not_wide, int32_t wide_max_nnz,
                              int short_wide, SpmmPlan *p, char *err, size_t err_len) {
    *p = SpmmPlan{};
    p->has_plan = has_plan;
    // SGC_SPMM_LIGHT_ORDER: plan = [n_heavy heavy rows | the other rows in
    // processing order] (taken before the hub split below moves the heavy rows)
    if ((flags & SGC_SPMM_LIGHT_ORDER) && has_plan) {
        if (n_heavy > n_rows) {
            snprintf(err, err_len, "%s: light order with n_heavy > rows", who);
            return SGC_EINVAL;
        }
        p->light_offset = n_heavy;
        p->n_light = n_rows - n_heavy;
    }
    const bool light_order = p->light_offset >= 0;
    // An accumulate launch leaves rows without nonzeros untouched, and the
    // plan is sorted longest first: with the plan's count of rows that have
    // nonzeros (n_nonempty >= 0; heavy rows are among them) the light items
    // stop where the empty rows begin -- no wave is started for them (the
    // multi-row kernel; the one-row kernel keeps row order over all rows,
    // spmm_schedule).  A plain launch covers every row (an empty row is written
    // as zeros).
    if (light_order && (flags & SGC_SPMM_ACCUMULATE) && n_nonempty >= 0) {
        if (!(n_nonempty >= n_heavy && n_nonempty <= n_rows)) {
            snprintf(err, err_len, "%s: n_nonempty %lld outside [n_heavy, rows]", who,
                     (long long)n_nonempty);
            return SGC_EINVAL;
        }
        p->n_light = n_nonempty - n_heavy;
    }
    // Wide items: the caller's count of light rows with more than
    // wide_max_nnz nonzeros (n_not_wide >= 0; the sorted plan lists them
    // first) leaves the rest of the light items -- in a plain launch the
    // rows without nonzeros too, written as zeros by the wide waves -- to
    // wide waves, where the launch can take them (spmm_schedule).
    if (light_order && n_not_wide >= 0 && short_wide != 0) {
        if (!(wide_max_nnz >= 1 && wide_max_nnz <= 32)) {
            snprintf(err, err_len, "%s: wide_max_nnz %d outside [1, 32]", who, wide_max_nnz);
            return SGC_EINVAL;
        }
        if (n_not_wide > n_rows - n_heavy) {
            snprintf(err, err_len, "%s: n_not_wide %lld > light rows", who, (long long)n_not_wide);
            return SGC_EINVAL;
        }
        p->n_wide = std::max<int64_t>(0, p->n_light - n_not_wide);
    }
    if (!has_plan) {
        n_heavy = 0;
        heavy_threshold = INT32_MAX;  // no plan: every row is a light item
    }
    n_hub = std::max<int64_t>(0, std::min<int64_t>(n_hub, n_heavy));
    if (flags & SGC_SPMM_NO_HUB) {  // hub rows are launched separately (SGC_SPMM_HUB_ONLY)
        p->heavy_skip = n_hub;
        n_heavy -= n_hub;
        n_hub = 0;
    }
    p->n_heavy = n_heavy;
    p->n_hub = n_hub;
    p->heavy_threshold = heavy_threshold;
    return SGC_OK;
}

// What the choice may look at.
struct SpmmShape {
    int64_t n_rows = 0, F = 0, ldx = 0, ldy = 0;
    uintptr_t x_addr = 0, y_addr = 0;  // alignment only
    uint32_t flags = 0;
    int32_t wide_max_nnz = 0;
    SpmmPlan plan;
};

enum SpmmHubMode {
    kHubNone = 0,    // no hub rows in this launch
    kHubConcurrent,  // spmm_hub_kernel on the caller's stream, the light kernel on a side stream
    kHubSerial,      // spmm_hub_kernel on the caller's stream before the light kernel (or alone: SGC_SPMM_HUB_ONLY)
    kHubFused        // hub items inside the light kernel's launch (HF = 32)
};

// Everything the launch step needs.
struct SpmmSchedule {
    // sgc_timing_collect_ex's code: 0 spmm_csr_kernel, 1 spmm_rows_kernel, 2 / 3
    // the same with the hub rows fused, -1 no light kernel (SGC_SPMM_HUB_ONLY)
    int kernel = -1;
    bool multi_row = false;  // spmm_rows_kernel<LB, VH, 16, O32, QV, HF, WD>, else spmm_csr_kernel<V, C, U, 16, HF>
    int V = 0, C = 0;        // one-row kernel: lane vector, chunks per slice
    int LB = 0, VH = 0, QV = 0, HF = 0, WD = 0;
    bool O32 = false;
    int LR = 0;         // multi-row kernel: lanes per row
    int F_load = 0;     // multi-row: F rounded up to 4; one-row: the kernel's F (padded with 16-B lanes)
    int vec_store = 0;  // multi-row: 16-B stores
    int slices = 0, n_sub = 0;
    int n_heavy = 0;        // heavy rows of the light kernel (the hub rows taken off)
    int n_light_items = 0;  // multi-row: light items per slice; one-row: every row
    int n_wide = 0, wide_first = 0;
    int64_t slice_blocks = 0, wide_blocks = 0;  // WD > 0: workgroups per slice, wide workgroups
    int64_t grid_x = 0;  // 0: nothing to launch (an accumulate launch over empty runs)
    int grid_y = 1;
    int kernel_bits = 0;  // the heavy_pairs bits (multi-row: 1 | 16; one-row: bit 1 as 1) and row_chunks_pipe2 as 2
    SpmmHubMode hub = kHubNone;
    int hub_chunk = 0, hub_loaders = 0;  // spmm_hub_kernel<hub_chunk, hub_loaders>
    int hub_n_chunks = 0;
    int64_t hub_grid = 0;
    int fused_chunks = 0, fused_blocks = 0;  // HF = 32: 32-float chunks per hub row, hub workgroups
};

inline int spmm_sched_fail(int code, char *err, size_t err_len, const char *msg) {
    snprintf(err, err_len, "%s", msg);
    return code;
}

// Largest per-lane register vector the strides and base pointers allow.
inline int spmm_pick_vec(const SpmmKnobs &k, int64_t F, int64_t ldx, int64_t ldy, uintptr_t xa,
                         uintptr_t ya) {
    for (int V : {4, 2}) {
        if (V <= k.max_vec && F % V == 0 && ldx % V == 0 && ldy % V == 0 && xa % (4 * V) == 0 &&
            ya % (4 * V) == 0)
            return V;
    }
    return 1;
}

// The choice.  sh.plan is spmm_plan_prologue's; sh.n_rows > 0.  Returns SGC_OK
// and *out, or the error code with its text in err.
inline int spmm_schedule(const SpmmShape &sh, const SpmmKnobs &k, SpmmSchedule *out, char *err,
                         size_t err_len) {
    SpmmSchedule s;
    const int64_t n_rows = sh.n_rows, F = sh.F, ldx = sh.ldx, ldy = sh.ldy;
    const uintptr_t xa = sh.x_addr, ya = sh.y_addr;
    const uint32_t flags = sh.flags;
    const int64_t n_hub = sh.plan.n_hub, n_wide = sh.plan.n_wide;
    int64_t n_heavy = sh.plan.n_heavy;
    const bool light_order = sh.plan.light_offset >= 0;
    const bool hub_only = (flags & SGC_SPMM_HUB_ONLY) != 0;
    const bool lines = ldx % 32 == 0 && xa % 128 == 0;
    // 32-feature chunks spread a hub over more CUs; measured faster up to
    // F = 160 and slower from F = 320 (scripts/sweep_narrow.py), and they
    // need 128-B aligned rows to stay one line per segment.
    s.hub_chunk = k.hub_chunk ? k.hub_chunk : (lines && F <= 192 ? 32 : 64);
    s.hub_loaders = k.hub_loaders == 7 ? 7 : 15;
    bool hub_deferred = false;  // serial hub rows left for the fused launch (or just before the light kernel)
    if (n_hub > 0) {
        // hub rows (the heaviest n_hub of the plan) run beside the light
        // kernel (hub_stream)
        if (!(n_hub * ((F + 31) / 32) < (int64_t)INT32_MAX))
            return spmm_sched_fail(SGC_ERANGE, err, err_len, "spmm: too many hub items");
        const bool serial =
            k.hub_stream == 2 || (k.hub_stream == 0 && (flags & SGC_SPMM_HUB_SERIAL));
        // (the fused items read floats one at a time: any row alignment)
        hub_deferred = serial && !hub_only && k.hub_fuse && k.hub_chunk == 0;
        s.hub = (!hub_only && !serial) ? kHubConcurrent : kHubSerial;
        s.hub_n_chunks = (int)((F + s.hub_chunk - 1) / s.hub_chunk);
        s.hub_grid = n_hub * s.hub_n_chunks;
        n_heavy -= n_hub;
        if (hub_only) {
            *out = s;
            return SGC_OK;
        }
    }
    s.n_heavy = (int)n_heavy;
    // 16-B lanes over F rounded up to 4 columns: X rows must be 16-B aligned
    // and readable that far (flag SGC_SPMM_X_PADDED unless F % 4 == 0)
    const int64_t F4 = (F + 3) / 4 * 4;
    const bool v4_ok = ldx % 4 == 0 && xa % 16 == 0 && F4 <= ldx && F4 >= 32 &&
                       (F4 == F || (flags & SGC_SPMM_X_PADDED));
    // With both buffers padded, the one-row kernel may compute F rounded up
    // to 4 as well: one 256-float slice (16-B lanes) covers a 129..256-float
    // launch that the multi-row kernel would run as two passes (128 + the
    // rest) -- e.g. a 146-column feature block at P = 4.  Wider launches keep
    // the multi-row kernel's 128-float slices (Reddit's 602: MALL residency).
    const bool pad_both = (flags & SGC_SPMM_X_PADDED) && (flags & SGC_SPMM_Y_PADDED);
    const int64_t F_csr =
        (F % 4 != 0 && pad_both && F4 > 128 && F4 <= 256 && F4 <= ldx && F4 <= ldy) ? F4 : F;
    const bool csr_v4 = F_csr % 4 == 0 && spmm_pick_vec(k, F_csr, ldx, ldy, xa, ya) == 4;
    // Small, wide launches (Cora shape: 2,708 rows x 1,433 features, X in
    // L2): latency-bound, so fewer and wider work items win -- the one-row
    // kernel with 512-float slices, 19.7 vs 24.9 us per hop for the
    // 128-float rows kernel (profiles/r02/small_shapes_sweep.log).  Only at
    // the default schedule knobs.
    const bool small_wide = n_rows * F <= (int64_t(1) << 23) && F > 256 && k.rows_per_wave == 0 &&
                            k.slice_floats == 128;
    const bool wide_rows = n_rows >= kWideRowsMin && (F4 == 128 || F4 > 256);
    s.multi_row = v4_ok && k.rows_per_wave != 1 && !small_wide &&
                  (k.rows_per_wave > 1 || !csr_v4 || F4 < 128 || wide_rows);
    if (s.multi_row) {
        s.F_load = (int)F4;
        s.vec_store = ldy % 4 == 0 && ya % 16 == 0 && F4 <= ldy &&
                      (F4 == F || (flags & SGC_SPMM_Y_PADDED));
        // lanes per row: the launch's width in 4-float lanes when it fits a
        // wave's half or less (one slice), else 32 (or 16 when forced)
        int LR = F4 >= 128 ? (k.rows_per_wave == 4 ? 16 : 32) : (int)(F4 / 4);
        if (LR > 32) LR = 32;
        s.LR = LR;
        const int SW = LR * 4;
        const bool multi = F4 > SW;
        const bool vh2 = F % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && xa % 8 == 0 &&
                         ya % 8 == 0 && (!multi || SW % (kSchedWave * 2) == 0);
        if (!(n_heavy * 8 + n_rows < (int64_t)INT32_MAX))
            return spmm_sched_fail(SGC_ERANGE, err, err_len, "spmm: too many work items");
        // the fused hub items need the 256-thread multi-row kernel with
        // 16-B lanes over whole slices (LR >= 16, two-float heavy sub-chunks)
        const bool fused = hub_deferred && LR >= 16 && vh2 && F4 > 64;
        s.kernel = fused ? 2 : 1;
        // 32-bit row offsets (one full-rate 24-bit multiply per gathered row)
        // when the caller vouches that X spans < 4 GiB and has < 2^24 rows
        s.O32 = (flags & SGC_SPMM_X_UNDER_4G) && ldx * 4 < (int64_t(1) << 24);
        // heavy rows four nonzeros per load (row_quads_pipe) on launches of at
        // most 32 floats; measured (one hop over all Reddit-shape rows,
        // interleaved, bit-identical, profiles/r04/quads_ab.log) 32 floats
        // 0.667 -> 0.615 ms, but 48 and 64 floats slower (0.68 -> 0.82, 0.72
        // -> 0.85) and 64-float slices at full width far slower (3.8 -> 5.8):
        // there the pairs stay
        int qv = ((k.heavy_pairs & 4) && LR <= 16 && F4 <= 32) ? (F4 > 16 ? 2 : 1) : 0;
        // 33..64 floats: the transposed quads (row_quadsT_pipe, heavy_pairs bit 8)
        if ((k.heavy_pairs & 8) && LR <= 16 && F4 > 32 && F4 <= 64) qv = 4;
        // wide items: 32 lanes per row over at least two slices, no fused
        // hub rows; the rule asks for a large launch, a forced Ts does not
        const bool wide = n_wide > 0 && LR == 32 && multi && !fused && qv == 0 &&
                          (k.short_wide > 0 || n_rows >= kWideRowsMin);
        s.QV = qv;
        s.HF = fused ? 32 : 0;
        // the light rows' LDS block: LB * rows per wave <= 64
        s.LB = (wide || fused || LR >= 16) ? 16 : 8;
        s.VH = (qv != 0 || fused || vh2) ? 2 : 1;
        s.WD = wide ? (sh.wide_max_nnz <= 16 ? 16 : 32) : 0;
        s.kernel_bits = k.heavy_pairs & 17;
        const int R = kSchedWave / LR;
        // each light row stages LB (col, val) pairs in its wave's 64-entry LDS block
        if (LR <= 0 || R * s.LB > kSchedWave)
            return spmm_sched_fail(SGC_EHIP, err, err_len, "spmm launch failed: invalid argument");
        s.slices = (int)((F4 + SW - 1) / SW);
        // heavy sub-chunks per slice (unpacked heavy rows): whole 64*VH-float
        // chunks of a slice, or of the launch's width when it is a single slice
        const int sub_floats = kSchedWave * s.VH;
        s.n_sub = (qv > 0 || (k.heavy_pairs & 1)) ? 1
                  : s.slices > 1 ? SW / sub_floats : (int)((F4 + sub_floats - 1) / sub_floats);
        const int64_t heavy_waves = n_heavy * s.n_sub;
        // light items: every row (non-light rows skip themselves), or with a
        // light order exactly the light rows (an accumulate launch: the light
        // rows with nonzeros, the order's head)
        const int64_t n_items = light_order ? sh.plan.n_light : n_rows;
        int64_t blocks;
        if (wide) {
            // a one-dimensional grid of the slices' workgroups in turn plus the
            // wide waves' workgroups, which replace the per-slice waves of the
            // last n_wide light items
            const int64_t n_narrow = n_items - n_wide;
            const int64_t waves = heavy_waves + (n_narrow + R - 1) / R;
            s.slice_blocks = (waves + kSchedWavesPerBlock - 1) / kSchedWavesPerBlock;
            const int64_t wide_waves = (n_wide + R - 1) / R;
            s.wide_blocks = (wide_waves + kSchedWavesPerBlock - 1) / kSchedWavesPerBlock;
            blocks = s.slice_blocks * s.slices + s.wide_blocks;
            if (n_narrow < 0)
                return spmm_sched_fail(SGC_EHIP, err, err_len,
                                       "spmm launch failed: invalid argument");
            s.n_light_items = (int)n_narrow;
            s.n_wide = (int)n_wide;
            s.wide_first = k.short_wide_first;
            s.grid_y = 1;
        } else {
            if (fused) {
                s.hub = kHubFused;
                s.fused_chunks = (int)((F + 31) / 32);
                s.fused_blocks = (int)(n_hub * s.fused_chunks);
            }
            const int64_t waves = heavy_waves + (n_items + R - 1) / R;
            blocks = (waves + kSchedWavesPerBlock - 1) / kSchedWavesPerBlock + s.fused_blocks;
            s.n_light_items = (int)n_items;
            s.grid_y = s.slices;
        }
        if (blocks >= INT32_MAX)
            return spmm_sched_fail(SGC_EHIP, err, err_len, "spmm launch failed: invalid argument");
        s.grid_x = blocks;
    } else {
        const int V = spmm_pick_vec(k, F_csr, ldx, ldy, xa, ya);
        s.V = V;
        s.F_load = (int)(V == 4 ? F_csr : F);  // pad columns only with 16-B lanes
        const int chunks_total = (s.F_load + kSchedWave * V - 1) / (kSchedWave * V);
        const int cmax = 16 / V;  // <= 16 accumulators per lane
        const int sf = small_wide ? 512 : k.slice_floats;
        int C = sf > 0 ? std::max(1, sf / (kSchedWave * V)) : cmax;
        C = std::min(C, std::min(cmax, chunks_total));
        s.C = C;
        s.slices = (chunks_total + C - 1) / C;
        s.VH = V < 2 ? V : 2;  // (SGC_HEAVY_VEC)
        if (!(n_heavy * (int64_t)C * V + n_rows < (int64_t)INT32_MAX))  // upper bound (VH >= 1)
            return spmm_sched_fail(SGC_ERANGE, err, err_len, "spmm: too many work items");
        if (!(s.slices < 65536))
            return spmm_sched_fail(SGC_ERANGE, err, err_len, "spmm: too many feature slices");
        // the fused hub items: the 16-B-lane, one-chunk slice form (Pubmed shape)
        const bool fused = hub_deferred && V == 4 && C == 1;
        s.kernel = fused ? 3 : 0;
        if (fused) {
            s.hub = kHubFused;
            s.HF = 32;
            s.fused_chunks = (int)((F + 31) / 32);
            s.fused_blocks = (int)(n_hub * s.fused_chunks);
        }
        // light items: every row in row order (non-light rows skip themselves),
        // accumulate launches too.  Taking an accumulate launch's light rows with
        // nonzeros from the plan instead (length order, as the multi-row kernel
        // does) measured slower here: RMAT shape, G = 4, one hop 29.29 -> 31.62 ms
        // in the pure split and 28.58 -> 28.63 with whole rows of <= 32 nonzeros
        // (profiles/whole_rows/sweep_rmat_allrows.log) -- a wave per row leaves
        // nothing to pack, and in row order the partial sums stream.
        s.n_light_items = (int)n_rows;
        s.n_sub = C * V / s.VH;
        const int64_t waves = n_heavy * s.n_sub + n_rows;
        const int64_t blocks =
            (waves + kSchedWavesPerBlock - 1) / kSchedWavesPerBlock + s.fused_blocks;
        if (blocks >= INT32_MAX)
            return spmm_sched_fail(SGC_EHIP, err, err_len, "spmm launch failed: invalid argument");
        s.grid_x = blocks;
        s.grid_y = s.slices;
        s.kernel_bits = ((k.heavy_pairs >> 1) & 1) | (n_rows >= kChunksPipe2Rows ? 2 : 0);
    }
    *out = s;
    return SGC_OK;
}

// "kernel<template arguments> LR= slices= n_sub= bits= grid= wide= hub=": what
// sgc_spmm_kernel_name returns.
inline void spmm_schedule_name(const SpmmSchedule &s, char *buf, size_t len) {
    static const char *const hub[] = {"none", "concurrent", "serial", "fused"};
    int n;
    if (s.kernel < 0)
        n = snprintf(buf, len, "none");
    else if (s.multi_row)
        n = snprintf(buf, len,
                     "spmm_rows_kernel<LB=%d,VH=%d,UH=16,O32=%d,QV=%d,HF=%d,WD=%d> LR=%d slices=%d "
                     "n_sub=%d bits=%d grid=%lldx%d wide=%d",
                     s.LB, s.VH, (int)s.O32, s.QV, s.HF, s.WD, s.LR, s.slices, s.n_sub,
                     s.kernel_bits, (long long)s.grid_x, s.grid_y, s.n_wide);
    else
        n = snprintf(buf, len,
                     "spmm_csr_kernel<V=%d,C=%d,UH=16,HF=%d> LR=0 slices=%d n_sub=%d bits=%d "
                     "grid=%lldx%d wide=0",
                     s.V, s.C, s.HF, s.slices, s.n_sub, s.kernel_bits, (long long)s.grid_x,
                     s.grid_y);
    if (n < 0 || (size_t)n >= len) return;
    if (s.hub == kHubConcurrent || s.hub == kHubSerial)
        snprintf(buf + n, len - n, " hub=%s spmm_hub_kernel<%d,%d> grid=%lld", hub[s.hub],
                 s.hub_chunk, s.hub_loaders, (long long)s.hub_grid);
    else
        snprintf(buf + n, len - n, " hub=%s", hub[s.hub]);
}

}  // namespace sgc
