// Host check of sgc_amd/csrc/lane_lines.h (compiled and run by
// test_lane_lines_host.py): enumerates every lane of every wave instruction
// of the SpMM kernels' lane -> column mappings and checks the invariant
//
//   whenever an instruction has an active lane, the 128-B lines its lanes
//   touch are a subset of the lines its ACTIVE lanes touch.
//
// The rule the kernels had before (idle lanes gather byte 0 of the gathered
// row) fails this at F = 602: in slice 4 of the multi-row mapping lanes
// 23..31 read line 0 while the active lanes read lines 16, 17 and 18.
#include <algorithm>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "lane_lines.h"

namespace {

constexpr int kWave = 64;
int g_fail = 0, g_instr = 0;

// (which gathered row / array, 128-B line within it)
typedef std::set<std::pair<int, long>> Lines;

void add_bytes(Lines &s, int which, long first, long bytes) {
    for (long b = first / 128; b <= (first + bytes - 1) / 128; ++b) s.insert({which, b});
}

void check(const Lines &all, const Lines &active, const char *what, int F, int a, int b) {
    ++g_instr;
    if (active.empty()) return;  // no active lane: nothing is promised
    if (!std::includes(active.begin(), active.end(), all.begin(), all.end())) {
        if (g_fail++ < 20)
            std::printf("FAIL %s F=%d (%d, %d): an idle lane touches a line no active lane reads\n",
                        what, F, a, b);
    }
}

// spmm_rows_kernel: LR lanes per row, 4 floats per lane, R = 64 / LR rows per
// wave (lanes past them alias row 0); heavy rows as pairs (lanes 0-31 one
// nonzero, lanes 32-63 the next) or four 16-lane groups.
void multi_row(int F) {
    const int V = 4, F_load = (F + 3) / 4 * 4;
    const int LR = F_load >= 128 ? 32 : F_load / 4, SW = LR * V, R = kWave / LR;
    const int slices = (F_load + SW - 1) / SW;
    for (int base = 0; base < 128; base += 16) {  // X rows are 16-B aligned
        for (int slice = 0; slice < slices; ++slice) {
            const int seg_end = std::min(F_load, (slice + 1) * SW);
            Lines all, act;
            for (int lane = 0; lane < kWave; ++lane) {  // light rows
                const int sub = lane / LR, l = lane - sub * LR;
                const int f = slice * SW + l * V;
                const bool ok = sub < R && f < seg_end;
                const int c = sgc::gather_col(f, seg_end, V);
                if (ok && c != f) ++g_fail;  // an active lane keeps its column
                const int row = sub < R ? sub : 0;
                add_bytes(all, row, base + 4L * c, 4 * V);
                if (ok) add_bytes(act, row, base + 4L * c, 4 * V);
            }
            check(all, act, "rows/light", F, slice, base);
            all.clear(), act.clear();
            for (int lane = 0; lane < kWave; ++lane) {  // pairs
                const int f = slice * SW + (lane & 31) * V;
                const bool ok = f < seg_end;
                const int c = sgc::gather_col(f, seg_end, V);
                if (ok && c != f) ++g_fail;
                add_bytes(all, lane >> 5, base + 4L * c, 4 * V);
                if (ok) add_bytes(act, lane >> 5, base + 4L * c, 4 * V);
            }
            check(all, act, "rows/pairs", F, slice, base);
            if (F_load > 64) continue;
            // quads: 16 lanes x QV floats (launches of <= 32 floats: QV = 2 / 1;
            // 33..64: 4, transposed)
            const int QV = F_load > 32 ? 4 : F_load > 16 ? 2 : 1;
            all.clear(), act.clear();
            for (int lane = 0; lane < kWave; ++lane) {
                const int f = slice * SW + (lane & 15) * QV;
                const bool ok = f < seg_end;
                const int c = sgc::gather_col(f, seg_end, QV);
                if (ok && c != f) ++g_fail;
                add_bytes(all, lane >> 4, base + 4L * c, 4 * QV);
                if (ok) add_bytes(act, lane >> 4, base + 4L * c, 4 * QV);
            }
            check(all, act, "rows/quads", F, slice, base);
        }
    }
}

// spmm_csr_kernel / row_chunks_pipe: one row per wave, lane l owns the V-float
// vectors at (chunk0 + c) * 64V + l * V, c in [0, C): one instruction per c.
// (V = 1 is also the hub loaders' and, per element, the 16-bit kernels' rule.)
void one_row(int F, int V) {
    for (int C = 1; C * V <= 16; C *= 2) {
        const int chunks = (F + kWave * V - 1) / (kWave * V);
        const int slices = (chunks + C - 1) / C;
        for (int base = 0; base < 128; base += 4 * V) {
            for (int slice = 0; slice < slices; ++slice) {
                for (int c = 0; c < C; ++c) {
                    Lines all, act;
                    for (int lane = 0; lane < kWave; ++lane) {
                        const int f = (slice * C + c) * (kWave * V) + lane * V;
                        const bool ok = f < F;
                        const int g = sgc::gather_col(f, F, V);
                        if (ok && g != f) ++g_fail;
                        if (g < 0 || g >= F) ++g_fail;  // never starts beyond the row
                        add_bytes(all, 0, base + 4L * g, 4 * V);
                        if (ok) add_bytes(act, 0, base + 4L * g, 4 * V);
                    }
                    check(all, act, "one-row", F, V * 100 + C, slice * 16 + c);
                }
            }
        }
    }
}

// The (col, val) staging loads of spmm_rows_kernel: lane l < LB of a row with
// nonzeros stages nonzero base + l (active); every other lane repeats one.
void staging(int LR, int LB, const std::vector<int> &lens) {
    const int R = kWave / LR;
    std::vector<int> k0(R), len(R);
    int k = 37, n_max = 0, k_max = 0;  // the wave's rows lie somewhere inside the CSR
    for (int s = 0; s < R; ++s) {
        len[s] = lens[s % lens.size()];
        k0[s] = k;
        k += len[s] + 3;
        if (len[s] > n_max) n_max = len[s], k_max = k0[s];
    }
    if (n_max == 0) return;  // the kernel stages nothing
    for (int base = 0; base < n_max + 2 * LB; base += LB) {
        Lines all, act;
        for (int lane = 0; lane < kWave; ++lane) {
            const int sub = lane / LR, l = lane - sub * LR;
            const int ln = sub < R ? len[sub] : 0, ks = sub < R ? k0[sub] : 0;
            const bool ok = sub < R && l < LB && ln > 0;
            const int k0_s = ln > 0 ? ks : k_max, len_s = ln > 0 ? ln : n_max;
            const int j = sgc::stage_index(base, l, LB, len_s);
            if (j < 0 || j >= len_s) ++g_fail;  // inside the row
            if (ok && j != std::min(base + l, ln - 1)) ++g_fail;
            add_bytes(all, 0, 4L * (k0_s + j), 4);
            if (ok) add_bytes(act, 0, 4L * (k0_s + j), 4);
        }
        check(all, act, "staging", LR, LB, base);
    }
}

}  // namespace

int main() {
    for (int F : {602, 516, 132, 130, 90, 76}) multi_row(F);
    for (int F : {64, 48, 36, 30, 12}) multi_row(F);  // the quads' widths
    for (int V : {1, 2, 4})
        for (int F : {500, 1433, 129, 127}) one_row(F, V);
    const std::vector<std::vector<int>> lens = {
        {40, 17, 5, 0}, {0, 0, 9, 1}, {16, 16, 16, 16}, {1, 0, 0, 0}, {0, 33, 0, 2}, {0, 0, 0, 0}};
    for (const auto &ls : lens) {
        staging(32, 16, ls);
        staging(16, 16, ls);
        staging(19, 16, ls);  // 76 floats: 3 rows per wave, 7 lanes of no row
        staging(8, 8, ls);
        staging(23, 16, ls);  // 90 floats
    }
    std::printf("%d instructions checked, %d failures\n", g_instr, g_fail);
    return g_fail ? 1 : 0;
}
