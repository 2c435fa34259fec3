// lane_lines.h -- where an idle lane of a gather instruction points.
//
// The SpMM kernels never predicate a load (a predicated load's phi copy waits
// for every load in flight), so lanes without work still execute every gather
// and every (col, val) staging load.  What such a lane costs is the 128-B line
// it touches: the rule here keeps it on a line that an active lane of the
// same instruction reads anyway, so an instruction touches no line the result
// does not need.  (Pointing idle lanes at feature 0 of the gathered row, as
// the kernels once did, added one line per nonzero to every ragged slice:
// at 602 floats slice 4 read lines 16, 17, 18 and line 0.)
//
// Plain functions, usable from host code too: tests/test_lane_lines_host.py
// enumerates every lane of every instruction with the host compiler.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SGC_LANE_FN __host__ __device__ __forceinline__
#else
#define SGC_LANE_FN inline
#endif

namespace sgc {

// First column of the V-wide vector a lane gathers.  `f` is the lane's own
// column (a multiple of V); `end` is where the instruction's valid columns
// stop: the launch's width, or the end of the lane group's segment when that
// comes first.  A lane with f < end is active and keeps f; an idle lane takes
// the last whole vector below `end`, which an active lane of the same
// instruction reads whenever the instruction has an active lane at all (its
// first column is then a multiple of V below `end`).  An instruction whose
// lanes all lie beyond `end` re-reads that vector: the previous chunk's last
// line, never a new one.  Needs end >= 1.
SGC_LANE_FN int gather_col(int f, int end, int V) {
    const int last = (end - 1) / V * V;
    return f < last ? f : last;
}

// Index, within its row, of the nonzero a lane of spmm_rows_kernel stages for
// the block that starts at nonzero `base`: lane l of the row's lanes stages
// nonzero base + l, clamped to the block (LB staged per row) and to the row's
// last nonzero.  `len` >= 1: a lane of an empty row, or of no row at all,
// passes the (k0, len) of a row of its wave that has nonzeros and so repeats
// an address one of that row's staging lanes reads.
SGC_LANE_FN int stage_index(int base, int l, int LB, int len) {
    const int j = base + (l < LB ? l : LB - 1);
    return j < len - 1 ? j : len - 1;
}

}  // namespace sgc
