// Host check of sgc_amd/csrc/spmm_schedule.h: the whole SpmmSchedule of every
// case of spmm_schedule_cases.inc against its literals (taken from launch_spmm
// as it was before the header existed), the prologue's error texts, and the
// name string.  Built by tests/test_spmm_schedule_host.py with the host C++
// compiler; exits non-zero on a mismatch and prints "N cases, M failures".
#include <cstdio>
#include <cstring>
#include <string>

#include "spmm_schedule.h"

using namespace sgc;

namespace {

constexpr int kFields = 31;

struct Case {
    const char *name;
    int64_t n_rows, F, ldx, ldy;
    unsigned long long x, y;
    uint32_t flags;
    int has_plan;
    int64_t n_heavy, n_hub;
    int32_t threshold;
    int64_t n_nonempty, n_not_wide;
    int32_t wide_max_nnz;
    int knobs[10];
    long long want[kFields];
};

const Case kCases[] = {
#include "spmm_schedule_cases.inc"
};

const char *const kFieldNames[kFields] = {
    "kernel", "multi_row", "V", "C", "LB", "VH", "QV", "HF", "WD", "O32", "LR", "F_load",
    "vec_store", "slices", "n_sub", "n_heavy", "n_light_items", "n_wide", "wide_first",
    "slice_blocks", "wide_blocks", "grid_x", "grid_y", "kernel_bits", "hub", "hub_chunk",
    "hub_loaders", "hub_n_chunks", "hub_grid", "fused_chunks", "fused_blocks"};

void fields(const SpmmSchedule &s, long long *f) {
    const long long v[kFields] = {
        s.kernel, s.multi_row, s.V, s.C, s.LB, s.VH, s.QV, s.HF, s.WD, s.O32, s.LR, s.F_load,
        s.vec_store, s.slices, s.n_sub, s.n_heavy, s.n_light_items, s.n_wide, s.wide_first,
        s.slice_blocks, s.wide_blocks, s.grid_x, s.grid_y, s.kernel_bits, s.hub, s.hub_chunk,
        s.hub_loaders, s.hub_n_chunks, s.hub_grid, s.fused_chunks, s.fused_blocks};
    std::memcpy(f, v, sizeof(v));
}

SpmmKnobs knobs_of(const int *k) {
    SpmmKnobs n;
    n.slice_floats = k[0], n.max_vec = k[1], n.rows_per_wave = k[2], n.heavy_pairs = k[3];
    n.hub_chunk = k[4], n.hub_stream = k[5], n.hub_loaders = k[6], n.hub_fuse = k[7];
    n.short_wide = k[8], n.short_wide_first = k[9];
    return n;
}

int failures = 0;

void expect(bool ok, const char *what, const char *detail = "") {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s %s\n", what, detail);
}

int run(const Case &c, SpmmSchedule *s, char *err, size_t n) {
    const SpmmKnobs k = knobs_of(c.knobs);
    SpmmShape sh;
    sh.n_rows = c.n_rows, sh.F = c.F, sh.ldx = c.ldx, sh.ldy = c.ldy;
    sh.x_addr = (uintptr_t)c.x, sh.y_addr = (uintptr_t)c.y;
    sh.flags = c.flags, sh.wide_max_nnz = c.wide_max_nnz;
    int rc = spmm_plan_prologue("spmm", c.n_rows, c.has_plan != 0, c.n_heavy, c.n_hub, c.threshold,
                                c.flags, c.n_nonempty, c.n_not_wide, c.wide_max_nnz, k.short_wide,
                                &sh.plan, err, n);
    if (rc != SGC_OK) return rc;
    return spmm_schedule(sh, k, s, err, n);
}

}  // namespace

int main() {
    char err[160];
    int n_cases = 0;
    for (const Case &c : kCases) {
        ++n_cases;
        SpmmSchedule s;
        err[0] = 0;
        const int rc = run(c, &s, err, sizeof(err));
        if (rc != SGC_OK) {
            expect(false, c.name, err);
            continue;
        }
        long long got[kFields];
        fields(s, got);
        for (int i = 0; i < kFields; ++i) {
            if (got[i] == c.want[i]) continue;
            char d[128];
            std::snprintf(d, sizeof(d), "%s: got %lld, want %lld", kFieldNames[i], got[i], c.want[i]);
            expect(false, c.name, d);
        }
    }

    // the defaults are the library's
    const SpmmKnobs def;
    expect(def.slice_floats == 128 && def.max_vec == 4 && def.rows_per_wave == 0 &&
               def.heavy_pairs == 29 && def.hub_chunk == 0 && def.hub_stream == 0 &&
               def.hub_loaders == 15 && def.hub_fuse == 1 && def.short_wide == -1 &&
               def.short_wide_first == 0,
           "default knobs");

    // the prologue's range checks and their texts, for both launchers' prefixes
    SpmmPlan p;
    const uint32_t order = SGC_SPMM_LIGHT_ORDER;
    expect(spmm_plan_prologue("spmm_x16", 10, true, 11, 0, 4, order, -1, -1, 0, 0, &p, err,
                              sizeof(err)) == SGC_EINVAL &&
               std::string(err) == "spmm_x16: light order with n_heavy > rows",
           "prologue: n_heavy > rows", err);
    expect(spmm_plan_prologue("spmm", 10, true, 3, 0, 4, order | SGC_SPMM_ACCUMULATE, 11, -1, 0, -1,
                              &p, err, sizeof(err)) == SGC_EINVAL &&
               std::string(err) == "spmm: n_nonempty 11 outside [n_heavy, rows]",
           "prologue: n_nonempty", err);
    expect(spmm_plan_prologue("spmm", 10, true, 3, 0, 4, order, -1, 2, 33, -1, &p, err,
                              sizeof(err)) == SGC_EINVAL &&
               std::string(err) == "spmm: wide_max_nnz 33 outside [1, 32]",
           "prologue: wide_max_nnz", err);
    expect(spmm_plan_prologue("spmm", 10, true, 3, 0, 4, order, -1, 8, 16, -1, &p, err,
                              sizeof(err)) == SGC_EINVAL &&
               std::string(err) == "spmm: n_not_wide 8 > light rows",
           "prologue: n_not_wide", err);
    // short_wide = 0 ignores the wide counts, bad ones included
    expect(spmm_plan_prologue("spmm", 10, true, 3, 0, 4, order, -1, 8, 33, 0, &p, err,
                              sizeof(err)) == SGC_OK && p.n_wide == 0,
           "prologue: short_wide off");
    // no plan: every row light, the counts dropped; NO_HUB skips the hub rows
    expect(spmm_plan_prologue("spmm", 10, false, 5, 2, 4, order, 7, 1, 16, -1, &p, err,
                              sizeof(err)) == SGC_OK &&
               p.n_heavy == 0 && p.n_hub == 0 && p.heavy_threshold == INT32_MAX &&
               p.light_offset == -1 && p.n_wide == 0,
           "prologue: no plan");
    expect(spmm_plan_prologue("spmm", 10, true, 5, 9, 4, order | SGC_SPMM_NO_HUB, -1, -1, 0, -1, &p,
                              err, sizeof(err)) == SGC_OK &&
               p.heavy_skip == 5 && p.n_heavy == 0 && p.n_hub == 0 && p.light_offset == 5 &&
               p.n_light == 5,
           "prologue: hub clamp and NO_HUB");

    // the name string (sgc_spmm_kernel_name) of the first case: Reddit, padded rows
    SpmmSchedule s;
    char name[256];
    if (run(kCases[0], &s, err, sizeof(err)) == SGC_OK) {
        spmm_schedule_name(s, name, sizeof(name));
        expect(std::string(name) ==
                   "spmm_rows_kernel<LB=16,VH=2,UH=16,O32=1,QV=0,HF=0,WD=0> LR=32 slices=5 "
                   "n_sub=1 bits=17 grid=30516x5 wide=0 hub=concurrent spmm_hub_kernel<64,15> grid=370",
               "name", name);
    } else {
        expect(false, "name", err);
    }

    std::printf("%d cases, %d failures\n", n_cases, failures);
    return failures != 0;
}
