"""Device CSR, SpMM and K-hop propagation on gfx950 through libsgc_amd.so.

This is the engine under the drop-in `sgc_precompute` (reference
utils.py:92-97).  Host code only marshals torch tensors into the C ABI
(include/sgc_amd.h); every byte of arithmetic runs in the HIP kernels for
ROCm tensors, and in the library's host twins (sgc_*_cpu, C++ threads) for
CPU tensors -- the reference's own CPU mode (args.py:39 --no-cuda).  A ROCm
tensor never takes the CPU path: mixed devices raise, as torch.spmm does.
"""
import os
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as _nnf

from . import _lib

# Schedule (results never depend on it; see sgc_plan_build): rows with more
# nonzeros than the heavy threshold are split into per-feature-chunk work
# items and scheduled first; rows above the hub threshold run on the LDS-
# staged hub kernel.  Both default to the launch's size, because what they
# bound is the tail -- one wave walking a long row with ~16 nonzeros in flight
# -- against the launch's duration (nnz x F bytes):
#   heavy = nnz*F / 2^23 to the nearest power of two, clamped to [64, 512];
#   hub   = max(heavy, nnz / 1024, 256), capped at 8,192 below 16 M nonzeros.
# The cap (round 2): half of Reddit (11.7 M nonzeros, a P = 2 rank) with
# nnz / 1024 = 11.4k leaves its ~11.5k-nonzero rows as one-wave heavy items
# whose latency outlasts the rank's slice passes -- 2.66 ms per hop vs 2.43
# with hubs above 8,192 (96 rows); the whole graph (19 vs 172 hubs) and a
# quarter (52 either way) are unchanged (profiles/r02/p24_hub_sweep.log).
# Measured (scripts/sweep_narrow.py, profiles/r01_heavy_threshold_sweep.log,
# r01_rank_work_threshold_sweep.log): Reddit full graph 512 / ~10 hubs (988
# hubs cost +20%); a 1/8 row block 128-256 / its 132 rows above 2,048
# (-25% vs. no hubs); Pubmed shape 64 / 16 hubs (-25% vs. 512); Cora shape
# 64 / no hubs (-50%: a 1024-thread hub block costs more than a ~170-nonzero
# row on one wave).  SGC_AMD_HEAVY_THRESHOLD / SGC_AMD_HUB_THRESHOLD pin them.
_HEAVY_ENV = os.environ.get("SGC_AMD_HEAVY_THRESHOLD")
DEFAULT_HEAVY_THRESHOLD = int(_HEAVY_ENV) if _HEAVY_ENV else None
_HUB_ENV = os.environ.get("SGC_AMD_HUB_THRESHOLD")
DEFAULT_HUB_THRESHOLD = int(_HUB_ENV) if _HUB_ENV else None
HUB_SHARE = 1024
HUB_CAP, HUB_CAP_BELOW_NNZ = 8192, 1 << 24


def auto_heavy_threshold(nnz_range, width):
    import math
    work = max(1.0, int(nnz_range) * max(1, int(width)) / float(1 << 23))
    return int(min(512, max(64, 1 << int(round(math.log2(work))))))


def auto_hub_threshold(nnz_range, heavy_threshold):
    hub = int(nnz_range) // HUB_SHARE
    if int(nnz_range) < HUB_CAP_BELOW_NNZ:
        hub = min(hub, HUB_CAP)
    return max(int(heavy_threshold), hub, 256)


class Plan(NamedTuple):
    rows: Optional[torch.Tensor]  # int32 heavy rows, heaviest first (None: no plan)
    n_heavy: int
    n_hub: int
    threshold: int
    max_hub_degree: int = 0  # nonzeros of the longest hub row (0: no hub rows)
    ordered: bool = False  # rows also lists the light rows, longest first (SPMM_LIGHT_ORDER)
    n_nonempty: int = -1  # rows with at least one nonzero (sgc_plan_sorted_ex); -1: not counted
    above: tuple = ()  # rows of more than 4 / 8 / 16 / 32 nonzeros (sgc_plan_sorted_ex2), heavy too

    @property
    def accumulate_light_items(self):
        """Light items of an SPMM_ACCUMULATE launch with this plan: the light
        rows that have nonzeros (the sorted plan's empty rows are its tail and
        get no wave), or None when the launch covers every row."""
        if not self.ordered or self.n_nonempty < 0:
            return None
        return self.n_nonempty - self.n_heavy

    def hub_flags(self):
        """The plan's launch flags: SPMM_HUB_SERIAL when the hub kernel is
        short enough to run in line, SPMM_LIGHT_ORDER when `rows` carries the
        light rows' order."""
        f = SPMM_HUB_SERIAL if 0 < self.max_hub_degree <= HUB_SERIAL_MAX_DEGREE else 0
        return f | (SPMM_LIGHT_ORDER if self.ordered else 0)


NO_PLAN = Plan(None, 0, 0, 0)

# Wide items (sgc_spmm_csr_f32_ex3, the "short_wide" knob of sgc_set_tuning): a
# light row of at most Ts nonzeros crosses every feature slice in one wave.
# The plan counts the rows above each candidate Ts, so the knob moves without
# a new plan; another forced Ts is counted from row_ptr once and cached.
SHORT_WIDE_CANDIDATES = (4, 8, 16, 32)


def short_wide_state():
    """(knob, Ts in force) of the wide items: sgc_get_tuning "short_wide" (-1 the
    rule, 0 off, 1..32 forced) and "short_wide_ts" (0 = off)."""
    state = int(_lib.load().sgc_get_tuning(b"short_wide_state"))  # (knob + 1) * 64 + Ts: one call
    return (state >> 6) - 1, state & 63


def wide_args(csr, pl, row_begin, row_end, ts=None):
    """(n_not_wide, wide_max_nnz) of sgc_spmm_csr_f32_ex3 for plan `pl` over rows
    [row_begin, row_end) of `csr` at the Ts in force (or `ts`): the plan's light
    rows with more than Ts nonzeros.  (-1, 0) -- no wide items -- when the
    knob is off or the plan is not the sorted one."""
    if ts is None:
        ts = short_wide_state()[1]
    if ts <= 0 or not pl.ordered or pl.n_nonempty < 0 or len(pl.above) != 4:
        return -1, 0
    if ts in SHORT_WIDE_CANDIDATES:
        above = pl.above[SHORT_WIDE_CANDIDATES.index(ts)]
    else:
        key = ("above", row_begin, row_end, ts)
        if key not in csr._plans:
            rp = csr.row_ptr[row_begin:row_end + 1]
            csr._plans[key] = int(((rp[1:] - rp[:-1]) > ts).sum().item())
        above = csr._plans[key]
    return max(0, above - pl.n_heavy), int(ts)

SLOT_FIXED, SLOT_X0, SLOT_OUT = 0, 1, 2  # sgc_launch_list_* pointer slots
SPMM_X_PADDED = 1  # sgc_spmm_csr_f32_ex flags (include/sgc_amd.h)
SPMM_Y_PADDED = 2
SPMM_NO_HUB = 4    # split launch: every row but the plan's hub rows
SPMM_HUB_ONLY = 8  # split launch: only the hub rows, on the current stream
SPMM_ACCUMULATE = 16  # column-block pass: continue the chains stored in out
SPMM_HUB_SERIAL = 32  # hub kernel before the light kernel on the same stream
SPMM_LIGHT_ORDER = 64  # plan rows = heavy rows + the light rows in processing order
SPMM_X_UNDER_4G = 128  # X spans < 4 GiB: the gathers may use 32-bit row offsets


def x_flags(X):
    """SPMM_X_UNDER_4G when X has < 2^24 rows and every row lies within 4 GiB
    of its first element (X.shape[0] is the CSR's column count, checked by
    the callers)."""
    n, ld = X.shape[0], X.stride(0)
    return SPMM_X_UNDER_4G if n < (1 << 24) and n * ld * 4 < (1 << 32) else 0
# Light rows of the multi-row kernel in length order (longest first), so the
# rows sharing a wavefront have about the same length: a wave runs to its
# longest row and the other rows' lanes re-load their last nonzero meanwhile
# (the texture-address unit is ~86% busy on the Reddit hop, so those loads
# cost time, profiles/r02/diag).  SGC_AMD_LIGHT_ORDER=0 keeps row order.
LIGHT_ORDER = os.environ.get("SGC_AMD_LIGHT_ORDER", "1") != "0"
# Longest hub row (nonzeros) for which the serial hub launch beats the
# side-stream fork/join: its chain (~6.4 ns per nonzero) plus a
# launch stays under the ~25 us the two cross-stream events cost.
HUB_SERIAL_MAX_DEGREE = 3072

STATUS_ROWS_SORTED = 1
STATUS_COLS_ASCENDING = 2
STATUS_OUT_OF_RANGE = 4

# Column groups (sgc_csr_colsplit): one hop as G launches over the same rows,
# group 0 plain and groups 1.. accumulating, each gathering only the X rows
# of its column range -- the live X slice is 1/G as large and more of it stays
# in the per-XCD L2s.  Same bits (rows with ascending columns only).  Measured
# one hop, interleaved, bit-identical (profiles/r03/s14/colgroup*.log):
# Reddit shape at 602 floats 4.30 -> 3.83 ms (G = 2; 3.81 at 3, 3.88 at 4, 4.73
# at 8), at 304 2.45 -> 2.29, at 128 0.95 -> 0.84, at 76 0.77 -> 0.77, at
# 152 / 256 (the one-row kernel) 1.56 -> 1.58 / 1.85 -> 1.88;
# RMAT shape (F = 256) 31.4 -> 30.1 (G = 2) -> 29.5 ms (G = 4).  None set =
# column_groups_for's size rule; SGC_AMD_COLUMN_GROUPS=G forces G (1 = off).
# Short rows are not cut (GROUP_WHOLE_ROWS below): the price of a group is per
# row, its gain per nonzero.
_GROUPS_ENV = os.environ.get("SGC_AMD_COLUMN_GROUPS")
COLUMN_GROUPS = int(_GROUPS_ENV) if _GROUPS_ENV else None
GROUPS_MIN_NNZ = 1 << 22    # below: latency-bound launches, one launch per hop
GROUPS_MIN_WIDTH = 128      # narrower launches gain nothing (76 floats: 0.77 vs 0.77 ms)
GROUPS_WIDE_NNZ = 1 << 26   # from here four groups (RMAT shape)
# Whole rows (sgc_csr_colsplit_ex): a row of at most T nonzeros is not cut; its
# whole run stays in group 0 and the accumulate launches skip it (the plan's
# count of rows with nonzeros bounds their light items).  A group costs per
# row and gains per gathered nonzero, and short rows are most rows but few
# nonzeros (Reddit shape: <= 32 nonzeros = 73 % of the rows, 5.9 % of the
# nonzeros).  Same bits.  Measured interleaved, every point bit-identical
# (scripts/whole_rows_ab.py, profiles/whole_rows/): Reddit shape, G = 2, the
# K = 2 step at T = 0 / 8 / 16 / 32 / 64 / 96: 7.98 / 7.71 / 7.61 / 7.60 / 7.65 /
# 7.80 ms (one hop at 602 floats 3.71 -> 3.59; the accumulate launch's light
# rows 201,713 -> 58,235); G = 3 is best at T = 16 (7.51) and G = 4 at T = 64
# (7.50), within 1.3 % of G = 2 at T = 32, so G stays.  RMAT shape, G = 4, the
# K = 3 step 88.15 / 85.77 / 85.54 / 85.64 / 85.72 / 86.16 ms (G = 2: 90.1 ->
# 89.0 at best).  T = 32 is the middle of both plateaus.  None = group_whole_rows_for's rule;
# SGC_AMD_GROUP_WHOLE_ROWS=T forces T (0 = the pure split).
_WHOLE_ENV = os.environ.get("SGC_AMD_GROUP_WHOLE_ROWS")
GROUP_WHOLE_ROWS = int(_WHOLE_ENV) if _WHOLE_ENV else None
GROUP_WHOLE_ROWS_RULE = 32
# Length ladder (sgc_csr_colsplit_ex2): the rows above T in two classes.  A
# heavy row (more than H nonzeros) is cut at all G column cuts; a medium row
# (T+1..H) only at the Gc coarse cuts (coarse cut j = fine cut j * G / Gc, its
# run stored in fine group j * G / Gc), so it keeps the runs it has today.
# Same bits.  Measured interleaved, every point bit-identical
# (scripts/group_ladder_ab.py, profiles/group_ladder/), T = 32 throughout:
# RMAT shape (F = 256, the one-row kernel), the K = 3 step at G = 4 uncut by
# class 85.45 ms; (G, Gc) = (8, 4) at H = 256 / 512 / 1024 / 2048: 80.39 /
# 80.38 / 83.74 / 89.16 -- the rows above 512 hold the nonzeros worth a finer
# cut, the plateau is 256..512, the rule takes H = 512.
# Reddit shape, the K = 2 step at 602 floats, G = 2 uncut by class 6.93 ms: the
# fine cut of the heavy rows alone LOSES -- (G, Gc, H) = (4, 2, 512) 7.13,
# (6, 2, 512) 7.07, (8, 2, 512) 7.15, (8, 2, 1024) 7.50, (3, 1, 512) 7.60,
# (6, 3, 512) 7.15, (8, 4, 512) 7.28; T = 16 / 64 move these by < 0.1.  A launch
# of 12.5 K heavy rows' runs alone is too short to fill the device, and the
# medium rows gain from the finer cut as well: (4, 2, 128) 6.79, (4, 2, 64)
# 6.77, every row above T cut four ways 6.77 (T = 16: 6.85, T = 64: 6.83),
# eight ways 7.10.  So at this shape the ladder's gain is the four-way cut of
# the rows above 64 (H = 64: the 15 K rows of 33..64 nonzeros keep runs of
# ~24 instead of ~12 at no cost in time); one hop at 304 floats it loses (1.94
# -> 2.01 ms; four ways uncut by class 1.98): a launch's fixed cost against a
# gain that grows with nnz x width.  Break-even by those two widths is about
# nnz x width = 9.4e9; the rule asks for GROUP_LADDER_MIN_WORK (1.18e10,
# Reddit shape at 602 floats is 1.41e10).
# GROUP_LADDER_RULE: the size rule's G (which stays the medium rows' Gc) ->
# (G, H).  SGC_AMD_GROUP_COARSE_GROUPS=Gc / SGC_AMD_GROUP_COARSE_ROWS=H force
# the two (Gc = G: no ladder); a forced SGC_AMD_COLUMN_GROUPS has no ladder
# unless Gc is forced too.
_COARSE_GROUPS_ENV = os.environ.get("SGC_AMD_GROUP_COARSE_GROUPS")
GROUP_COARSE_GROUPS = int(_COARSE_GROUPS_ENV) if _COARSE_GROUPS_ENV else None
_COARSE_ROWS_ENV = os.environ.get("SGC_AMD_GROUP_COARSE_ROWS")
GROUP_COARSE_ROWS = int(_COARSE_ROWS_ENV) if _COARSE_ROWS_ENV else None
GROUP_COARSE_ROWS_RULE = 512
GROUP_LADDER_RULE = {2: (4, 64), 4: (8, 512)}  # the size rule's G (= Gc) -> (fine G, H)
GROUP_LADDER_MIN_WORK = 11 << 30  # nnz x width below which Gc = 2 keeps G = 2


def group_whole_rows_for(csr, G):
    """T of the whole-row rule for G column groups of `csr`."""
    if G <= 1:
        return 0
    if GROUP_WHOLE_ROWS is not None:
        return max(0, int(GROUP_WHOLE_ROWS))
    return GROUP_WHOLE_ROWS_RULE


def _size_rule_groups(csr, width):
    """The size rule's coarse cut: the column groups every row above T had
    before the length ladder (and the medium rows still have)."""
    if width < GROUPS_MIN_WIDTH or csr.nnz < GROUPS_MIN_NNZ:
        return 1
    if csr.nnz >= GROUPS_WIDE_NNZ:
        return 4
    if 128 < width <= 256:  # the one-row kernel's single 256-float slice: no gain
        return 1            # (152 floats 1.56 -> 1.58 ms, 256 1.85 -> 1.88 at G = 2)
    return 2


def group_coarse_for(csr, G):
    """(Gc, H) of the length ladder for G column groups of `csr`: rows of more
    than H nonzeros are cut at all G cuts, rows of T+1..H at the Gc coarse
    ones.  Gc == G: no ladder.  A forced G (COLUMN_GROUPS) has no ladder unless
    GROUP_COARSE_GROUPS asks for one; a Gc that does not divide G is ignored."""
    T = group_whole_rows_for(csr, G)
    if G <= 1:
        return 1, 0
    Gc, H = G, GROUP_COARSE_ROWS_RULE
    if COLUMN_GROUPS is None:  # the rule's G: its coarse cut is the size rule's
        coarse = 4 if csr.nnz >= GROUPS_WIDE_NNZ else 2
        fine, rows = GROUP_LADDER_RULE.get(coarse, (coarse, H))
        if fine == G:
            Gc, H = coarse, rows
    if GROUP_COARSE_GROUPS is not None and G % max(1, int(GROUP_COARSE_GROUPS)) == 0:
        Gc = max(1, int(GROUP_COARSE_GROUPS))
    if GROUP_COARSE_ROWS is not None:
        H = int(GROUP_COARSE_ROWS)
    return (Gc, max(H, T)) if Gc != G else (G, T)


def group_ladder_for(csr, width):
    """(G, Gc, H) for a plain launch of `width` features over `csr`: G column
    groups, of which rows of at most H nonzeros take only the Gc coarse cuts
    (Gc == G: every row above T is cut alike, H unused)."""
    if csr.device.type != "cuda" or not csr.cols_ascending or csr.nnz == 0:
        return 1, 1, 0
    if COLUMN_GROUPS is not None:
        G = max(1, min(8, int(COLUMN_GROUPS), max(1, csr.n_cols)))
    else:
        G = _size_rule_groups(csr, width)
        # the ladder where it was measured to win: the one-row kernel's
        # widths at four coarse groups, enough work per launch at two
        measured = {4: 128 < width <= 256, 2: csr.nnz * width >= GROUP_LADDER_MIN_WORK}
        if measured.get(G):
            G = GROUP_LADDER_RULE.get(G, (G,))[0]
    return (G, *group_coarse_for(csr, G))


def column_groups_for(csr, width):
    """Column groups (launches per hop) for a plain launch of `width`
    features over `csr`: the G of group_ladder_for."""
    return group_ladder_for(csr, width)[0]


def _host_cols_ascending(row_ptr, col_idx):
    """Every row's columns strictly ascending?  (host arrays; False for
    anything else, which only turns the column groups off)."""
    if isinstance(row_ptr, torch.Tensor):
        if row_ptr.device.type != "cpu" or col_idx.device.type != "cpu":
            return False
        row_ptr, col_idx = row_ptr.numpy(), col_idx.numpy()
    rp = np.asarray(row_ptr, dtype=np.int64)
    ci = np.asarray(col_idx)
    if ci.size < 2:
        return True
    bad = np.diff(ci.astype(np.int64)) <= 0  # bad[k-1]: col[k] <= col[k-1]
    starts = rp[1:-1]
    starts = starts[(starts > 0) & (starts < ci.size)]
    bad[starts - 1] = False  # k is a row's first nonzero: no predecessor in its row
    return not bool(bad.any())


def _require_device(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"sgc_amd: {what} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"sgc_amd: {what} is on {t.device}; the propagation engine runs only on a "
            "ROCm (gfx950) device -- move tensors with .cuda() (no CPU fallback)")


def cpu_threads():
    """Threads of the host path: torch's intra-op setting (torch.set_num_threads)."""
    return max(1, torch.get_num_threads())


@dataclass
class DeviceCSR:
    """int32 CSR of the normalised adjacency S, resident in HBM (or in host
    memory for a CPU adjacency).

    Built once per adjacency tensor (cached on it) by a stable sort of the
    COO entries by row: every stored entry is kept and each row keeps its
    storage order, which is the FMA order of torch.spmm's CPU kernel."""
    n_rows: int
    n_cols: int
    row_ptr: torch.Tensor  # int32 [n_rows+1]
    col_idx: torch.Tensor  # int32 [nnz]
    val: torch.Tensor      # float32 [nnz]
    status: int = 0
    ingest_seconds: float = 0.0
    _plans: dict = field(default_factory=dict)

    @property
    def nnz(self):
        return self.col_idx.numel()

    @property
    def device(self):
        return self.row_ptr.device

    @property
    def cols_ascending(self):
        """Every row's columns strictly ascending (the ingest's status bit)."""
        return bool(self.status & STATUS_COLS_ASCENDING)

    def group_cuts(self, G):
        """Column cuts of the G column groups: group g = columns [c_g, c_{g+1})."""
        return [(g * self.n_cols) // G for g in range(G + 1)]

    def column_groups(self, G, whole_rows=0, coarse_rows=None, coarse_groups=None):
        """The G column-group CSRs of this one (sgc_csr_colsplit_ex2; cached):
        columns cut at g * n_cols / G, every row's run of each group in its
        storage order; group g's row_ptr points into one shared col/val
        copy.  A row of at most `whole_rows` nonzeros is not cut: all of it
        is in group 0 (0 = the pure split).  With `coarse_groups` = Gc
        dividing G, a row of at most `coarse_rows` nonzeros is cut only at
        every (G / Gc)-th cut, its runs in groups 0, G / Gc, ... (None = G:
        every cut row is cut at all the cuts).  Rows must have ascending
        columns."""
        if not self.cols_ascending:
            raise ValueError("sgc_amd: column groups need rows with ascending columns")
        whole_rows = int(whole_rows)
        if whole_rows < 0:
            raise ValueError("sgc_amd: whole_rows must be >= 0")
        whole_rows = min(whole_rows, 2 ** 31 - 1)
        G = int(G)
        coarse_groups = G if coarse_groups is None else int(coarse_groups)
        if coarse_groups < 1 or G % coarse_groups:
            raise ValueError(f"sgc_amd: coarse_groups {coarse_groups} must divide G = {G}")
        if coarse_groups == G or coarse_rows is None:  # no medium class: one cache entry
            coarse_groups, coarse_rows = G, whole_rows
        coarse_rows = min(int(coarse_rows), 2 ** 31 - 1)
        if coarse_rows < whole_rows:
            raise ValueError("sgc_amd: coarse_rows must be >= whole_rows")
        key = ("groups", G, whole_rows)
        if coarse_groups != G:
            key += (coarse_rows, coarse_groups)
        if key not in self._plans:
            import ctypes
            lib = _lib.load()
            n, nnz, dev = self.n_rows, self.nnz, self.device
            cuts = (ctypes.c_int32 * (G + 1))(*self.group_cuts(G))
            row_ptrs = torch.empty((G, n + 1), dtype=torch.int32, device=dev)
            col = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)
            val = torch.empty(max(1, nnz), dtype=torch.float32, device=dev)
            ws_bytes = lib.sgc_colsplit_workspace(n, G)
            ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.sgc_csr_colsplit_ex2(_lib.ptr(self.row_ptr),
                                                    _lib.ptr(self.col_idx), _lib.ptr(self.val), n,
                                                    self.n_cols, G,
                                                    ctypes.cast(cuts, ctypes.c_void_p), whole_rows,
                                                    coarse_rows, coarse_groups,
                                                    _lib.ptr(row_ptrs), _lib.ptr(col),
                                                    _lib.ptr(val), _lib.ptr(ws), ws_bytes,
                                                    _lib.stream_handle(dev)), "csr_colsplit")
            del ws  # stream-ordered: the allocator reuses it after the kernels
            self._plans[key] = [DeviceCSR(n, self.n_cols, row_ptrs[g], col[:nnz], val[:nnz],
                                          self.status) for g in range(G)]
        return self._plans[key]

    def release_prepared(self):
        """Free propagate()'s recorded launch lists on this adjacency (each
        keeps its launches' arguments and up to PREPARED_LOOP_MAX_BYTES of
        intermediates; at most PREPARED_LOOPS_KEPT of them).  The next call
        records again."""
        for key in [k for k in self._plans if isinstance(k, tuple) and k[:1] == ("list",)]:
            del self._plans[key]

    def drop_groups(self):
        """Free the cached column-group copies of S (and their plans): one
        more col/val copy per (G, whole_rows, coarse_rows, coarse_groups) (188
        MB at Reddit shape; propagate() under the rules uses one).  They
        are rebuilt on the next launch that uses them."""
        self.release_prepared()  # recorded launch lists hold the groups' pointers
        for key in [k for k in self._plans if isinstance(k, tuple) and k[:1] == ("groups",)]:
            for part in self._plans.pop(key):
                part._plans.clear()

    def groups_or_self(self, G):
        """The G column-group CSRs under the whole-row rule
        (group_whole_rows_for) and the length ladder (group_coarse_for), or
        [self] when G == 1 or when the copy does not fit in device memory (a
        schedule: the results are the same)."""
        if G <= 1:
            return [self]
        try:
            Gc, H = group_coarse_for(self, G)
            return self.column_groups(G, group_whole_rows_for(self, G), H, Gc)
        except torch.cuda.OutOfMemoryError:
            return [self]

    @classmethod
    def from_host_arrays(cls, row_ptr, col_idx, val, n_cols=None, device="cuda"):
        """From host CSR arrays already in the SpMM's order (numpy or torch)."""
        status = STATUS_COLS_ASCENDING if _host_cols_ascending(row_ptr, col_idx) else 0
        rp = torch.as_tensor(row_ptr).to(device=device, dtype=torch.int32)
        ci = torch.as_tensor(col_idx).to(device=device, dtype=torch.int32)
        va = torch.as_tensor(val).to(device=device, dtype=torch.float32)
        n = rp.numel() - 1
        return cls(n, n if n_cols is None else n_cols, rp.contiguous(), ci.contiguous(),
                   va.contiguous(), status)

    @classmethod
    def from_torch(cls, adj):
        """From a torch sparse COO (reference utils.py:23-30 layout) or CSR tensor."""
        import time
        if isinstance(adj, torch.Tensor) and adj.device.type == "cpu":
            return cls._from_torch_cpu(adj)
        _require_device(adj, "adj")
        if adj.dtype != torch.float32:
            raise TypeError(f"sgc_amd: adj must be float32, got {adj.dtype}")
        if adj.dim() != 2:
            raise ValueError("sgc_amd: adj must be 2-D")
        lib = _lib.load()
        n_rows, n_cols = adj.shape
        dev = adj.device
        t0 = time.perf_counter()
        with torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)
            status = _lib._u32(0)
            if adj.layout == torch.sparse_coo:
                idx = adj._indices().contiguous()
                vals = adj._values().contiguous()
                nnz = vals.numel()
                rows, cols = idx[0], idx[1]
                row_ptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
                col_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
                val = torch.empty(nnz, dtype=torch.float32, device=dev)
                ws_bytes = _lib._sz(0)
                _lib.check(lib.sgc_coo_to_csr_workspace(n_rows, nnz, ctypes_byref(ws_bytes)),
                           "coo_to_csr_workspace")
                ws = torch.empty(max(1, ws_bytes.value), dtype=torch.uint8, device=dev)
                _lib.check(lib.sgc_coo_to_csr(_lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), nnz,
                                              n_rows, n_cols, _lib.ptr(row_ptr), _lib.ptr(col_idx),
                                              _lib.ptr(val), _lib.ptr(ws), ws_bytes.value,
                                              ctypes_byref(status), stream), "coo_to_csr")
                del ws
            elif adj.layout == torch.sparse_csr:
                crow = adj.crow_indices().to(torch.int64).contiguous()
                ccol = adj.col_indices().to(torch.int64).contiguous()
                vals = adj.values().contiguous()
                nnz = vals.numel()
                row_ptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
                col_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
                val = torch.empty(nnz, dtype=torch.float32, device=dev)
                _lib.check(lib.sgc_csr64_to_csr(_lib.ptr(crow), _lib.ptr(ccol), _lib.ptr(vals),
                                                nnz, n_rows, n_cols, _lib.ptr(row_ptr),
                                                _lib.ptr(col_idx), _lib.ptr(val),
                                                ctypes_byref(status), stream), "csr64_to_csr")
            else:
                raise TypeError(f"sgc_amd: unsupported adj layout {adj.layout}")
        csr = cls(n_rows, n_cols, row_ptr, col_idx, val, int(status.value))
        csr.ingest_seconds = time.perf_counter() - t0
        return csr

    @classmethod
    def _from_torch_cpu(cls, adj):
        """Host CSR of a CPU adjacency (sgc_coo_to_csr_cpu: stable by row)."""
        import time
        if adj.dtype != torch.float32:
            raise TypeError(f"sgc_amd: adj must be float32, got {adj.dtype}")
        if adj.dim() != 2:
            raise ValueError("sgc_amd: adj must be 2-D")
        lib = _lib.load()
        n_rows, n_cols = adj.shape
        t0 = time.perf_counter()
        if adj.layout == torch.sparse_coo:
            idx = adj._indices().contiguous()
            vals = adj._values().contiguous()
        elif adj.layout == torch.sparse_csr:
            crow = adj.crow_indices().to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(n_rows, dtype=torch.int64),
                                           crow[1:] - crow[:-1])
            idx = torch.stack([rows, adj.col_indices().to(torch.int64)])
            vals = adj.values().contiguous()
        else:
            raise TypeError(f"sgc_amd: unsupported adj layout {adj.layout}")
        nnz = vals.numel()
        row_ptr = torch.empty(n_rows + 1, dtype=torch.int32)
        col_idx = torch.empty(nnz, dtype=torch.int32)
        val = torch.empty(nnz, dtype=torch.float32)
        status = _lib._u32(0)
        _lib.check(lib.sgc_coo_to_csr_cpu(_lib.ptr(idx[0]), _lib.ptr(idx[1]), _lib.ptr(vals), nnz,
                                          n_rows, n_cols, _lib.ptr(row_ptr), _lib.ptr(col_idx),
                                          _lib.ptr(val), ctypes_byref(status)), "coo_to_csr_cpu")
        csr = cls(n_rows, n_cols, row_ptr, col_idx, val, int(status.value))
        csr.ingest_seconds = time.perf_counter() - t0
        return csr

    def range_nnz(self, row_begin, row_end):
        """Nonzeros of rows [row_begin, row_end) (cached; reads row_ptr once)."""
        key = ("nnz", row_begin, row_end)
        if key not in self._plans:
            nnz = 0
            if row_end > row_begin:
                ends = self.row_ptr[[row_begin, row_end]].tolist()
                nnz = ends[1] - ends[0]
            self._plans[key] = nnz
        return self._plans[key]

    def plan(self, row_begin=0, row_end=None, threshold=None, hub_threshold=None,
             width=None) -> Plan:
        """Heavy-row schedule for rows [row_begin, row_end) at `width` features
        (cached).  Thresholds left None take the size-based defaults above."""
        row_end = self.n_rows if row_end is None else row_end
        if threshold is None:
            threshold = DEFAULT_HEAVY_THRESHOLD
        if threshold is None:
            threshold = auto_heavy_threshold(self.range_nnz(row_begin, row_end),
                                             width if width is not None else 512)
        threshold = int(threshold)
        hub = DEFAULT_HUB_THRESHOLD if hub_threshold is None else int(hub_threshold)
        if hub is None:
            hub = auto_hub_threshold(self.range_nnz(row_begin, row_end), threshold)
        hub = max(hub, threshold)
        key = (row_begin, row_end, threshold, hub)
        if key not in self._plans and LIGHT_ORDER and self.device.type == "cuda":
            self._plans[key] = self._plan_sorted(row_begin, row_end, threshold, hub)
        if key not in self._plans:
            lib = _lib.load()
            n = row_end - row_begin
            cap = lib.sgc_plan_capacity(n)
            buf = torch.empty(max(1, cap), dtype=torch.int32, device=self.device)
            n_heavy, n_hub = _lib._i64(0), _lib._i64(0)
            with torch.cuda.device(self.device):
                _lib.check(lib.sgc_plan_build(_lib.ptr(self.row_ptr), row_begin, row_end, threshold,
                                              hub, _lib.ptr(buf), cap, ctypes_byref(n_heavy),
                                              ctypes_byref(n_hub),
                                              _lib.stream_handle(self.device)), "plan_build")
            h, nh = int(n_heavy.value), int(n_hub.value)
            deg = 0
            if nh > 0:  # heaviest first: row 0 of the plan is the longest hub chain
                r = int(buf[0].item())
                ends = self.row_ptr[[r, r + 1]].tolist()
                deg = ends[1] - ends[0]
            rows, ordered = buf[:max(h, 1)].clone(), False
            if LIGHT_ORDER and self.device.type == "cuda" and n > h:
                # plan rows = [heavy rows | light rows longest first]
                rows = torch.empty(n, dtype=torch.int32, device=self.device)
                rows[:h].copy_(buf[:h])
                n_light = _lib._i64(0)
                with torch.cuda.device(self.device):
                    _lib.check(lib.sgc_plan_light_order(
                        _lib.ptr(self.row_ptr), row_begin, row_end, threshold,
                        _lib.ptr(rows[h:]), ctypes_byref(n_light),
                        _lib.stream_handle(self.device)), "plan_light_order")
                if int(n_light.value) != n - h:
                    raise RuntimeError("sgc_amd: light order does not cover the light rows")
                ordered = True
            self._plans[key] = Plan(rows, h, nh, threshold, deg, ordered)
        return self._plans[key]


    def _plan_sorted(self, row_begin, row_end, threshold, hub):
        """The plan from one device radix sort (sgc_plan_sorted): all rows of
        the range by degree, longest first -- heavy rows, then the light rows
        in processing order -- and the counts in one read-back."""
        import ctypes
        lib = _lib.load()
        n = row_end - row_begin
        rows = torch.empty(max(1, n), dtype=torch.int32, device=self.device)
        ws_bytes = lib.sgc_plan_sorted_workspace(n)
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=self.device)
        counts = (ctypes.c_int64 * 8)()
        with torch.cuda.device(self.device):
            _lib.check(lib.sgc_plan_sorted_ex2(_lib.ptr(self.row_ptr), row_begin, row_end,
                                               threshold, hub, _lib.ptr(rows), _lib.ptr(ws),
                                               ws_bytes, ctypes.cast(counts, ctypes.c_void_p),
                                               _lib.stream_handle(self.device)), "plan_sorted")
        h, nh = int(counts[0]), int(counts[1])
        return Plan(rows, h, nh, threshold, int(counts[2]) if nh > 0 else 0, n > h,
                    int(counts[3]), tuple(int(c) for c in counts[4:8]))


def to_torch_coo(csr: DeviceCSR):
    """torch sparse COO (int64 [2, nnz] indices, fp32 values, not coalesced) with
    the entries in CSR order -- the tensor sparse_mx_to_torch_sparse_tensor
    (utils.py:23-30) builds -- with `csr` attached as its propagation cache."""
    lib = _lib.load()
    nnz = csr.nnz
    idx = torch.empty((2, nnz), dtype=torch.int64, device=csr.device)
    if nnz > 0:  # an empty S (every row summing to 0) has no index storage to fill
        with torch.cuda.device(csr.device):
            _lib.check(lib.sgc_csr_to_coo64(_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx),
                                            csr.n_rows, _lib.ptr(idx[0]), _lib.ptr(idx[1]),
                                            _lib.stream_handle(csr.device)), "csr_to_coo64")
    adj = torch.sparse_coo_tensor(idx, csr.val, (csr.n_rows, csr.n_cols))
    try:
        adj._sgc_amd_csr = (adj._version, csr)
    except (AttributeError, RuntimeError):
        pass
    return adj


def ctypes_byref(x):
    import ctypes
    return ctypes.byref(x)


def csr_of(adj):
    """Cached DeviceCSR of a torch sparse adjacency (rebuilt if adj changed)."""
    cached = getattr(adj, "_sgc_amd_csr", None)
    if cached is not None and cached[0] == adj._version:
        return cached[1]
    csr = DeviceCSR.from_torch(adj)
    try:
        adj._sgc_amd_csr = (adj._version, csr)
    except (AttributeError, RuntimeError):
        pass
    return csr


# 16-bit feature storage (sgc_spmm_csr_x16: 16 bits in memory, the fp32 FMA
# chains in registers, one round-to-nearest-even per stored element).
X16_DTYPES = {torch.bfloat16: 1, torch.float16: 2}  # -> SGC_DTYPE_* (include/sgc_amd.h)


def is_x16(X):
    return isinstance(X, torch.Tensor) and X.dtype in X16_DTYPES


def require_f32_features(X, what):
    """The paths that only exist for fp32 features refuse 16-bit ones loudly
    (none of them may run an fp32 kernel over 16-bit memory)."""
    if is_x16(X):
        raise TypeError(f"sgc_amd: {what} supports float32 features only, got {X.dtype}: "
                        "16-bit features run through spmm / propagate / sgc_precompute on "
                        "one GPU (or the CPU)")


def _sgc_dtype(dtype):
    return 0 if dtype == torch.float32 else X16_DTYPES[dtype]


def aligned_ld_x16(F):
    """Row stride (elements) of the engine's own 16-bit feature buffers: 128-B rows."""
    return (F + 63) // 64 * 64


def _needs_pad_x16(X):
    return X.stride(0) % 64 != 0 or X.data_ptr() % 128 != 0


def x16_flags(X):
    """SPMM_X_UNDER_4G for a 16-bit X: < 2^24 rows, all within 4 GiB."""
    n, ld = X.shape[0], X.stride(0)
    return SPMM_X_UNDER_4G if n < (1 << 24) and n * ld * 2 < (1 << 32) else 0


def _out_dtype16(X, out, out_dtype):
    """The output type of a 16-bit launch: X's, or float32."""
    want = out.dtype if out is not None and out_dtype is None else out_dtype
    want = X.dtype if want is None else want
    if want not in (X.dtype, torch.float32):
        raise TypeError(f"sgc_amd: {X.dtype} features give {X.dtype} or float32 output, "
                        f"not {want}")
    if out is not None and out.dtype != want:
        raise TypeError(f"sgc_amd: out is {out.dtype}, out_dtype {want}")
    return want


def _spmm_cpu_x16(csr, X, row_begin, row_end, out, flags):
    """The definition itself on CPU tensors: the host twin on X.float(), then
    one rounding to the output type (none for float32)."""
    lib = _lib.load()
    Xf = X.float().contiguous()
    F = X.shape[1]
    if flags & SPMM_HUB_ONLY:
        return out
    acc = out if out.dtype == torch.float32 else torch.empty((row_end - row_begin, F),
                                                             dtype=torch.float32)
    _lib.check(lib.sgc_spmm_csr_f32_cpu_ex(_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx),
                                           _lib.ptr(csr.val), row_begin, row_end, _lib.ptr(Xf),
                                           Xf.stride(0), _lib.ptr(acc), acc.stride(0), F,
                                           int(flags) & SPMM_ACCUMULATE, cpu_threads()),
               "spmm_csr_f32_cpu")
    if acc is not out:
        out.copy_(acc)  # torch's CPU conversion: round to nearest even
    return out


def _spmm_x16(csr, X, row_begin, row_end, out, use_plan, threshold, hub_threshold, flags,
              out_dtype):
    F = X.shape[1]
    want = _out_dtype16(X, out, out_dtype)
    if flags & SPMM_ACCUMULATE and want != torch.float32:
        raise TypeError("sgc_amd: SPMM_ACCUMULATE needs a float32 out (a chain carried through "
                        "a 16-bit store would not be exact)")
    if out is None:
        if flags & SPMM_ACCUMULATE:
            raise ValueError("sgc_amd: SPMM_ACCUMULATE continues the chains in `out`; pass it")
        out = torch.empty((row_end - row_begin, F), dtype=want, device=X.device)
    if out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (row_end - row_begin, F):
        raise RuntimeError("sgc_amd: out must be [rows, F] with unit column stride")
    if F == 0 or row_end == row_begin:
        return out
    if X.device.type == "cpu":
        return _spmm_cpu_x16(csr, X, row_begin, row_end, out, flags)
    lib = _lib.load()
    with torch.cuda.device(X.device):
        pl = csr.plan(row_begin, row_end, threshold, hub_threshold, F) if use_plan else NO_PLAN
        _lib.check(lib.sgc_spmm_csr_x16(_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx),
                                        _lib.ptr(csr.val), row_begin, row_end, _lib.ptr(X),
                                        _sgc_dtype(X.dtype), X.stride(0), _lib.ptr(out),
                                        _sgc_dtype(out.dtype), out.stride(0), F,
                                        _lib.ptr(pl.rows), pl.n_heavy, pl.n_hub, pl.threshold,
                                        int(flags) | pl.hub_flags() | x16_flags(X),
                                        _lib.stream_handle(X.device)), "spmm_csr_x16")
    return out


def _propagate_x16(csr, X, K, out, use_plan, threshold, hub_threshold, hop_hook, out_dtype):
    """propagate() for bfloat16 / float16 features: X_{k+1} = fp32_spmm(S,
    X_k.float()).to(T) bit for bit; the last hop writes X's dtype or, with
    out_dtype=torch.float32, its unrounded fp32 chains.  One launch per hop:
    column groups would need ACCUMULATE through an fp32 buffer."""
    n, F = X.shape
    want = _out_dtype16(X, out, out_dtype)
    if out is None:
        out = torch.empty((n, F), dtype=want, device=X.device)
    if out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (n, F):
        raise RuntimeError("sgc_amd: out must be [N, F] with unit column stride")
    if n == 0 or F == 0:
        return out
    if X.device.type == "cpu":
        src = X
        for h in range(K):
            dst = out if h == K - 1 else torch.empty((n, F), dtype=X.dtype)
            _spmm_cpu_x16(csr, src, 0, n, dst, 0)
            src = dst
        return out
    lib = _lib.load()
    stream = torch.cuda.current_stream(X.device).cuda_stream
    pl = csr.plan(0, n, threshold, hub_threshold, F) if use_plan else NO_PLAN
    ldw = aligned_ld_x16(F)
    with torch.cuda.device(X.device):
        # the 2-byte re-layout's copy moves 4 B per element against 64 B per
        # nonzero saved, the same ratio as pad_pays' fp32 rule
        pad = _needs_pad_x16(X) and (pad_pays(csr, F) if PAD_X0 is None else bool(PAD_X0))
        n_bufs = min(2, int(pad) + min(K - 1, 2))
        bufs = [torch.empty((n, ldw), dtype=X.dtype, device=X.device) for _ in range(n_bufs)]
        src, nxt = X, 0
        if pad:
            bufs[0][:, :F].copy_(X)  # (a torch strided copy)
            src, nxt = bufs[0][:, :F], 1 % len(bufs)
        for h in range(K):
            dst = out if h == K - 1 else bufs[nxt][:, :F]
            # the engine's own buffers may be read / written in their pad columns
            flags = ((SPMM_X_PADDED if src is not X else 0) |
                     (SPMM_Y_PADDED if dst is not out else 0) | x16_flags(src) | pl.hub_flags())
            if hop_hook:
                hop_hook("start", h)
            _lib.check(lib.sgc_spmm_csr_x16(_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx),
                                            _lib.ptr(csr.val), 0, n, _lib.ptr(src),
                                            _sgc_dtype(src.dtype), src.stride(0), _lib.ptr(dst),
                                            _sgc_dtype(dst.dtype), dst.stride(0), F,
                                            _lib.ptr(pl.rows), pl.n_heavy, pl.n_hub,
                                            pl.threshold, flags, stream), "spmm_csr_x16")
            if hop_hook:
                hop_hook("end", h)
            src, nxt = dst, nxt ^ 1
    return out


def _check_features(X, csr):
    if not isinstance(X, torch.Tensor):
        raise TypeError("sgc_amd: features must be a torch.Tensor")
    if csr.device.type != "cpu":
        _require_device(X, "features")
    if X.device != csr.device:
        raise RuntimeError(f"sgc_amd: features on {X.device} but adj on {csr.device}")
    if X.dtype != torch.float32 and X.dtype not in X16_DTYPES:
        raise TypeError(f"sgc_amd: features must be float32, got {X.dtype} "
                        "(bfloat16 / float16 features: spmm, propagate, sgc_precompute)")
    if X.dim() != 2 or X.shape[0] != csr.n_cols:
        raise RuntimeError(f"sgc_amd: size mismatch, adj {csr.n_rows}x{csr.n_cols} . "
                           f"features {tuple(X.shape)}")
    if X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        X = X.contiguous()
    return X


def check_propagation_inputs(csr: DeviceCSR, X: torch.Tensor):
    """The checks propagate() makes (types, devices, shapes, a square S);
    returns X with unit column stride."""
    X = _check_features(X, csr)
    if csr.n_rows != csr.n_cols:
        raise RuntimeError("sgc_amd: propagation needs a square adjacency")
    return X


def spmm(csr: DeviceCSR, X: torch.Tensor, row_begin=0, row_end=None, out=None,
         use_plan=True, threshold=None, hub_threshold=None, flags=0, out_dtype=None):
    """One hop Y = S[row_begin:row_end] . X (bit-exact with torch.spmm on CPU).
    flags: SPMM_* bits of sgc_spmm_csr_f32_ex (a split launch on the GPU: NO_HUB
    / HUB_ONLY; on the CPU the whole hop runs for the NO_HUB part and nothing
    for HUB_ONLY, so the two parts still write every row once; ACCUMULATE
    continues the FMA chains already in `out`, which must then be given).
    bfloat16 / float16 X (sgc_spmm_csr_x16): the same fp32 chains on the
    widened elements, rounded once into X's dtype -- or stored unrounded with
    out_dtype=torch.float32 (the only output ACCUMULATE continues)."""
    X = _check_features(X, csr)
    row_end = csr.n_rows if row_end is None else row_end
    F = X.shape[1]
    if is_x16(X):
        return _spmm_x16(csr, X, row_begin, row_end, out, use_plan, threshold, hub_threshold,
                         flags, out_dtype)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"sgc_amd: float32 features give float32 output, not {out_dtype}")
    if out is None:
        if flags & SPMM_ACCUMULATE:
            raise ValueError("sgc_amd: SPMM_ACCUMULATE continues the chains in `out`; pass it")
        out = torch.empty((row_end - row_begin, F), dtype=torch.float32, device=X.device)
    if F == 0 or row_end == row_begin:
        return out
    lib = _lib.load()
    if X.device.type == "cpu":
        if flags & SPMM_HUB_ONLY:
            return out
        _lib.check(lib.sgc_spmm_csr_f32_cpu_ex(_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx),
                                               _lib.ptr(csr.val), row_begin, row_end,
                                               _lib.ptr(X), X.stride(0), _lib.ptr(out),
                                               out.stride(0), F, int(flags) & ~SPMM_NO_HUB,
                                               cpu_threads()), "spmm_csr_f32_cpu")
        return out
    G = 1
    if use_plan and not flags & (SPMM_ACCUMULATE | SPMM_NO_HUB | SPMM_HUB_ONLY):
        G = column_groups_for(csr, F)
    parts = csr.groups_or_self(G)
    with torch.cuda.device(X.device):
        stream = _lib.stream_handle(X.device)
        for g, c in enumerate(parts):  # group 0 plain, groups 1.. continue its chains
            pl = c.plan(row_begin, row_end, threshold, hub_threshold, F) if use_plan else NO_PLAN
            args = spmm_args(c, pl, row_begin, row_end, X, out,
                             int(flags) | pl.hub_flags() | x_flags(X) |
                             (SPMM_ACCUMULATE if g else 0), wide_args(c, pl, row_begin, row_end))
            _lib.check(lib.sgc_spmm_csr_f32_ex3(*args, stream), "spmm_csr_f32")
    return out


def spmm_args(csr, pl, row_begin, row_end, X, out, flags, wide):
    """The arguments of sgc_spmm_csr_f32_ex3 before its stream (and of
    sgc_launch_list_add_spmm_ex3 between its handle and its slots): CSR `csr`
    with plan `pl` over rows [row_begin, row_end), X -> out, `wide` =
    wide_args()'s (n_not_wide, wide_max_nnz)."""
    return (_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx), _lib.ptr(csr.val), int(row_begin),
            int(row_end), _lib.ptr(X), X.stride(0), _lib.ptr(out), out.stride(0), X.shape[1],
            _lib.ptr(pl.rows), pl.n_heavy, pl.n_hub, pl.threshold, int(flags), pl.n_nonempty,
            *wide)


class SpmmLaunch:
    """One prepared SpMM launch (fixed CSR, plan, X, out, flags): the ctypes
    arguments are built once and each call only passes the stream.  The
    multi-GPU pipeline replays a dozen launches per step, where the checks
    and lookups of spmm() would cost more host time than the launches take on
    the GPU.  The tensors must stay alive and unchanged in shape/storage;
    keep_tensors=False drops the references to X and out (for caches keyed by
    their data_ptr/shape/stride, which only replay a launch for live tensors
    at those addresses -- so a cache never pins a caller's tensor)."""

    __slots__ = ("_fn", "_args", "_keep")

    def __init__(self, csr: DeviceCSR, X: torch.Tensor, out: torch.Tensor, row_begin=0,
                 row_end=None, flags=0, threshold=None, hub_threshold=None, keep_tensors=True):
        X = _check_features(X, csr)
        require_f32_features(X, "SpmmLaunch (prepared launches)")
        if X.device.type != "cuda":
            raise RuntimeError("SpmmLaunch: ROCm tensors only")
        row_end = csr.n_rows if row_end is None else row_end
        F = X.shape[1]
        pl = csr.plan(row_begin, row_end, threshold, hub_threshold, F)
        lib = _lib.load()
        self._fn = lib.sgc_spmm_csr_f32_ex3
        self._keep = (csr, X, out, pl) if keep_tensors else (csr, pl)
        self._args = spmm_args(csr, pl, row_begin, row_end, X, out,
                               int(flags) | pl.hub_flags() | x_flags(X),
                               wide_args(csr, pl, int(row_begin), int(row_end)))

    def __call__(self, stream_handle):
        rc = self._fn(*self._args, stream_handle)
        if rc:
            _lib.check(rc, "spmm_csr_f32 (prepared)")


def aligned_ld(F):
    """Row stride (floats) of the engine's own feature buffers: 128-B rows."""
    return (F + 31) // 32 * 32


def _needs_pad(X):
    return X.stride(0) % 32 != 0 or X.data_ptr() % 128 != 0


# Override of pad_pays (None = the rule; True / False force the re-layout on
# or off -- scripts/pad_ab.py times both, results bit-identical either way).
PAD_X0 = None


def pad_pays(csr, F):
    """Re-lay X_0 into 128-B rows before hop 1?  An unaligned row segment
    touches about one extra 128-B line per gathered row (32/F of the hop's
    gather bytes, 128 B per nonzero); the copy moves 8 B per element of X
    (read + write).  With gathers ~1.2x the streaming rate the copy pays when
    16 * nnz/N > 1.2 F: Reddit (degree 100, F 602) and RMAT shape yes,
    Pubmed / Cora shape (degree ~5) no."""
    n = max(1, csr.n_rows)
    return 16.0 * csr.range_nnz(0, csr.n_rows) / n > 1.2 * F


def propagate(csr: DeviceCSR, X: torch.Tensor, K: int, out=None, use_plan=True, threshold=None,
              hop_hook=None, native_loop=False, hub_threshold=None, prepare=True, out_dtype=None):
    """X_K = S^K X on the device (K >= 1); asynchronous on the current stream.

    Mirrors sgc_propagate_f32: X is first re-laid into 128-B aligned rows when
    its rows are not and the copy pays (pad_pays: one streaming copy; each
    gathered X segment then spans the fewest 128-B lines -- sgc_propagate_f32
    always copies), hops ping-pong between two aligned buffers, the
    last hop writes the contiguous [N, F] result.  hop_hook(phase, h) is called
    around each hop's launch ("start"/"end", for event timing).
    native_loop=True runs the same loop inside the C ABI call instead.
    prepare=False neither replays nor records a launch list (GraphedPropagation's
    warm-up and capture; nothing is kept under a stream capture either).
    bfloat16 / float16 X: hops ping-pong between two 16-bit buffers (rows of
    aligned_ld_x16(F) elements), each hop one sgc_spmm_csr_x16 launch, every
    hop's fp32 chains rounded once into X's dtype; out_dtype=torch.float32
    makes the last hop store its chains unrounded.  No launch list, native
    loop or column groups there.  K <= 0 returns X itself."""
    X = check_propagation_inputs(csr, X)
    n, F = X.shape
    if is_x16(X):
        if native_loop:
            require_f32_features(X, "propagate(native_loop=True)")
        if K <= 0:
            return X
        return _propagate_x16(csr, X, K, out, use_plan, threshold, hub_threshold, hop_hook,
                              out_dtype)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"sgc_amd: float32 features give float32 output, not {out_dtype}")
    if out is None:
        out = torch.empty((n, F), dtype=torch.float32, device=X.device)
    if n == 0 or F == 0 or K <= 0:
        if K <= 0:
            out.copy_(X)
        return out
    lib = _lib.load()
    if X.device.type == "cpu":  # host twin (reference CPU mode), same bits
        ws_bytes = lib.sgc_propagate_cpu_workspace(n, F, int(K))
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8)
        _lib.check(lib.sgc_propagate_f32_cpu(_lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx),
                                             _lib.ptr(csr.val), n, _lib.ptr(X), X.stride(0),
                                             _lib.ptr(out), out.stride(0), F, int(K), _lib.ptr(ws),
                                             ws_bytes, cpu_threads()), "propagate_f32_cpu")
        return out
    stream = torch.cuda.current_stream(X.device).cuda_stream  # (an int: ctypes takes it as void *)
    G_rule = column_groups_for(csr, F) if use_plan else 1
    wide_knob, wide_ts = short_wide_state()
    # small launches (Cora / Pubmed shape: 20-40 us hops) pay their host time:
    # the loop's launches are recorded once per (shape, strides, X_0's 128-B
    # alignment, K, stream, schedule) into a native launch list, with the
    # intermediates kept beside it, and replayed by one call that takes this
    # call's X_0 and X_K
    key = None
    if (not native_loop and hop_hook is None and prepare and X.data_ptr() != out.data_ptr()
            and not torch.cuda.is_current_stream_capturing()):
        key = ("list", X.stride(0), F, int(K), out.stride(0), X.data_ptr() % 128 == 0,
               threshold, hub_threshold, bool(use_plan), G_rule,
               group_whole_rows_for(csr, G_rule), group_coarse_for(csr, G_rule), stream, PAD_X0,
               wide_knob, wide_ts)
        prep = csr._plans.get(key)
        if prep is not None:
            rc = lib.sgc_launch_list_run(prep[1].handle, X.data_ptr(), out.data_ptr(), stream)
            if rc:
                _lib.check(rc, "propagate (launch list)")
            return out
    groups = csr.groups_or_self(G_rule)
    G = len(groups)
    if G > 1:
        pl = None
        parts = [(c, c.plan(0, n, threshold, hub_threshold, F)) for c in groups]
    else:
        pl = csr.plan(0, n, threshold, hub_threshold, F) if use_plan else NO_PLAN
        parts = [(csr, pl)]
    # (csr, plan, launch flags of the group): groups 1.. continue group 0's chains
    parts = [(c, cp, cp.hub_flags() | (SPMM_ACCUMULATE if g else 0))
             for g, (c, cp) in enumerate(parts)]
    wide = [wide_args(c, cp, 0, n, wide_ts) for c, cp, _ in parts]
    ldw = aligned_ld(F)
    with torch.cuda.device(X.device):
        if native_loop:  # the same loop inside one C ABI call (sgc_propagate_groups_f32)
            import ctypes
            Gn = len(parts)
            ws_bytes = lib.sgc_propagate_workspace(n, F, X.stride(0), K)
            ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=X.device)
            planned = use_plan and all(cp.rows is not None for _, cp, _ in parts)
            plans = (ctypes.c_void_p * Gn)(*[cp.rows.data_ptr() if planned else None
                                             for _, cp, _ in parts])
            n_heavy = (ctypes.c_int64 * Gn)(*[cp.n_heavy for _, cp, _ in parts])
            n_hub = (ctypes.c_int64 * Gn)(*[cp.n_hub for _, cp, _ in parts])
            ths = (ctypes.c_int32 * Gn)(*[cp.threshold for _, cp, _ in parts])
            pflags = (ctypes.c_uint32 * Gn)(*[cp.hub_flags() for _, cp, _ in parts])
            nonempty = (ctypes.c_int64 * Gn)(*[cp.n_nonempty for _, cp, _ in parts])
            not_wide = (ctypes.c_int64 * Gn)(*[w[0] for w in wide])
            row_ptrs = parts[0][0].row_ptr  # groups: row 0 of the [G, n+1] row_ptrs tensor
            _lib.check(lib.sgc_propagate_groups_f32_ex3(
                Gn, _lib.ptr(row_ptrs), _lib.ptr(parts[0][0].col_idx), _lib.ptr(parts[0][0].val), n,
                _lib.ptr(X), X.stride(0), _lib.ptr(out), out.stride(0), F, int(K),
                ctypes.cast(plans, ctypes.c_void_p) if planned else None,
                ctypes.cast(n_heavy, ctypes.c_void_p), ctypes.cast(n_hub, ctypes.c_void_p),
                ctypes.cast(ths, ctypes.c_void_p), ctypes.cast(pflags, ctypes.c_void_p),
                ctypes.cast(nonempty, ctypes.c_void_p), ctypes.cast(not_wide, ctypes.c_void_p),
                max(w[1] for w in wide), _lib.ptr(ws), ws_bytes, stream), "propagate_groups_f32")
            return out
        pad = _needs_pad(X) and (pad_pays(csr, F) if PAD_X0 is None else bool(PAD_X0))
        # buffers actually used: the re-laid X_0 (if any) + up to two
        # ping-pong intermediates (the last hop writes `out`)
        n_bufs = min(2, int(pad) + min(K - 1, 2))
        prepared = key is not None and n_bufs * n * ldw * 4 <= PREPARED_LOOP_MAX_BYTES
        bufs = [torch.empty((n, ldw), dtype=torch.float32, device=X.device)
                for _ in range(n_bufs)]
        ops = []  # the launches as recorded: (kind, args without the stream, src slot, dst slot)

        def slot(t):
            return SLOT_X0 if t is X else SLOT_OUT if t is out else SLOT_FIXED
        src, nxt = X, 0
        if pad:
            args = (_lib.ptr(X), X.stride(0), _lib.ptr(bufs[0]), ldw, n, F)
            ops.append(("pad", args, SLOT_X0, SLOT_FIXED))
            src, nxt = bufs[0][:, :F], 1 % len(bufs)
            _lib.check(lib.sgc_pad_rows_f32(*args, stream), "pad_rows_f32")
        for h in range(K):
            dst = out if h == K - 1 else bufs[nxt][:, :F]
            # the engine's own buffers may be read / written in their pad columns
            flags = ((SPMM_X_PADDED if src is not X else 0) |
                     (SPMM_Y_PADDED if dst is not out else 0) | x_flags(src))
            if hop_hook:
                hop_hook("start", h)
            for (c, cp, gflags), w in zip(parts, wide):  # column groups: 0 plain, 1.. accumulate
                args = spmm_args(c, cp, 0, n, src, dst, flags | gflags, w)
                ops.append(("spmm", args, slot(src), slot(dst)))
                _lib.check(lib.sgc_spmm_csr_f32_ex3(*args, stream), "spmm_csr_f32")
            if hop_hook:
                hop_hook("end", h)
            src, nxt = dst, nxt ^ 1
        if prepared:
            old = [k for k in csr._plans if isinstance(k, tuple) and k[:1] == ("list",)]
            for k in old[:max(0, len(old) - PREPARED_LOOPS_KEPT + 1)]:
                del csr._plans[k]  # oldest first (dicts keep insertion order)
            csr._plans[key] = (bufs, LaunchList(ops), parts)  # parts: keep the pointers alive
    return out


class LaunchList:
    """A native launch list (sgc_launch_list_*) holding one propagate() loop:
    the ops as recorded, X_0 / X_K by slot; destroyed with this object."""

    __slots__ = ("handle", "_lib")

    def __init__(self, ops):
        import ctypes
        lib = _lib.load()
        h = ctypes.c_int64(0)
        _lib.check(lib.sgc_launch_list_create(ctypes.byref(h)), "launch_list_create")
        self.handle, self._lib = h.value, lib
        for kind, args, s_src, s_dst in ops:
            if kind == "pad":
                rc = lib.sgc_launch_list_add_pad_rows(self.handle, *args, s_src, s_dst)
            else:
                rc = lib.sgc_launch_list_add_spmm_ex3(self.handle, *args, s_src, s_dst)
            _lib.check(rc, "launch_list_add")

    def __del__(self):
        try:
            if self.handle:
                self._lib.sgc_launch_list_destroy(self.handle)
                self.handle = 0
        except Exception:  # interpreter shutdown: the library may be gone
            pass


# propagate()'s recorded launch lists: at most this many bytes of intermediates each,
# and this many (X, out, K, stream) combinations per adjacency
PREPARED_LOOP_MAX_BYTES = 1 << 26
PREPARED_LOOPS_KEPT = 4


class GraphedPropagation:
    """The K-hop loop of propagate() captured once into a HIP graph, for
    repeated propagation over one adjacency at one feature shape (many feature
    sets, serving, hyper-parameter sweeps like the reference's tuning.py).

    It makes the whole loop -- pad copy, K SpMM launches, the hub kernels'
    fork/join on the side stream -- one replayable unit, e.g. inside a larger
    captured serving step.  It is not a speed-up on its own: even at Pubmed
    shape a hop is GPU-bound, and a replay measured 118 us against 122 us
    eager at K=2, the static-input copy included
    (profiles/r01_bench_small_v2.log).  run(X) copies X into the graph's static
    input and replays; the result is in self.out (bit-identical to
    propagate()).
    Capture builds the plan first (it synchronises) and warms the code
    objects on a side stream, as torch.cuda.graph requires."""

    def __init__(self, csr: DeviceCSR, shape, K: int, threshold=None, hub_threshold=None):
        n, F = shape
        if K < 1:
            raise ValueError("GraphedPropagation: K >= 1")
        self.csr, self.K = csr, int(K)
        self.x_in = torch.empty((n, F), dtype=torch.float32, device=csr.device)
        self.out = torch.empty((n, F), dtype=torch.float32, device=csr.device)
        self.x_in.zero_()
        kw = dict(threshold=threshold, hub_threshold=hub_threshold)
        csr.plan(0, n, threshold, hub_threshold, F)  # synchronous: never inside the capture
        side = torch.cuda.Stream(device=csr.device)
        side.wait_stream(torch.cuda.current_stream(csr.device))
        with torch.cuda.stream(side):  # (no launch list kept for the side stream)
            propagate(csr, self.x_in, self.K, out=self.out, prepare=False, **kw)
        torch.cuda.current_stream(csr.device).wait_stream(side)
        torch.cuda.synchronize(csr.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            propagate(csr, self.x_in, self.K, out=self.out, prepare=False, **kw)

    def run(self, X: torch.Tensor) -> torch.Tensor:
        X = _check_features(X, self.csr)
        require_f32_features(X, "GraphedPropagation")
        if tuple(X.shape) != tuple(self.x_in.shape):
            raise RuntimeError(f"GraphedPropagation: captured for {tuple(self.x_in.shape)}, "
                               f"got {tuple(X.shape)}")
        self.x_in.copy_(X)
        self.graph.replay()
        return self.out


WARM_PROPAGATE, WARM_CLASSIFIER, WARM_LOADERS = 1, 2, 4  # sgc_warmup units (sgc_amd.h)
_warmed = {}


def warmup(device=None, units=WARM_PROPAGATE | WARM_CLASSIFIER):
    """Load the library's code objects on `device` now (sgc_warmup: one empty
    launch per translation unit), once per process and device, so that the
    first sgc_precompute a caller times (reddit.py:43,72-74) does not pay
    them.  The loaders call it when they move data to the GPU.  Returns the
    seconds it took (0.0 when already done)."""
    import time
    d = torch.device("cuda") if device is None else torch.device(device)
    dev = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
    key = (dev.index, int(units))
    if key in _warmed:
        return 0.0
    lib = _lib.load()
    t = time.perf_counter()
    with torch.cuda.device(dev):
        _lib.check(lib.sgc_warmup(int(units), _lib.stream_handle(dev)), "warmup")
        if units & WARM_PROPAGATE:
            # one tiny propagation through the same steps as sgc_precompute's
            # one-GPU path, so the torch kernels they use (COO accessors,
            # indexing, allocation) load here as well; the COO is row-unsorted
            # (the ingest's sort runs too).  No process-group step: under
            # torchrun every rank warms on its own.
            n = 64
            i = torch.arange(n, device=dev)
            idx = torch.stack([torch.cat([(i + 1) % n, i]), torch.cat([i, i])])
            adj = torch.sparse_coo_tensor(idx, torch.full((2 * n,), 0.5, device=dev), (n, n))
            csr = csr_of(adj)
            propagate(csr, torch.ones((n, 8), device=dev), 2)
            # the multi-GPU partitions' device-built shards (searchsorted,
            # indexing, casts): their torch kernels' first use cost the first
            # P = 4 call ~0.2 s of its 0.42 (profiles/r06/s20)
            from .distributed import _chunk_order, make_shard_device
            make_shard_device(csr, 1, 3)
            _chunk_order(csr, [(0, 32), (32, n)])
        torch.cuda.synchronize(dev)
        if units & WARM_PROPAGATE:
            # torch's stream pool for this device (the multi-GPU partitions'
            # chunk / tail streams): its first use creates the pool's streams,
            # new hardware queues among them (~8 ms each, profiles/r06/s10)
            torch.cuda.Stream(device=dev)
            # under torchrun: the process group the partitioned sgc_precompute
            # uses is set up here, with the loaders (rendezvous and RCCL's
            # communicator, eagerly bound to this device), not inside the
            # first call the reference times (reddit.py:43)
            from . import multigpu
            multigpu.process_group(dev)
    _warmed[key] = time.perf_counter() - t
    return _warmed[key]


def kernel_timing(on: bool):
    """Turn per-kernel launch timing on/off (sgc_timing_enable; diagnostics)."""
    _lib.check(_lib.load().sgc_timing_enable(1 if on else 0), "timing_enable")


def collect_kernel_timing(capacity=1 << 16):
    """(light_ms, hub_ms) lists of the SpMM launches recorded since the last
    collect; hub_ms[i] is None for a launch without hub rows (synchronous)."""
    import ctypes
    lib = _lib.load()
    light = (ctypes.c_float * capacity)()
    hub = (ctypes.c_float * capacity)()
    n = _lib._i64(0)
    _lib.check(lib.sgc_timing_collect(ctypes.cast(light, ctypes.c_void_p),
                                      ctypes.cast(hub, ctypes.c_void_p), capacity,
                                      ctypes_byref(n)), "timing_collect")
    k = int(n.value)
    return [float(light[i]) for i in range(k)], [float(hub[i]) if hub[i] >= 0 else None
                                                 for i in range(k)]


def collect_launch_timing(capacity=1 << 16):
    """Per SpMM launch since the last collect: (light_ms, hub_ms, span_ms,
    light_kernel) lists -- span = the whole launch as the caller's stream
    sees it (hub kernel joined); light_kernel = "spmm_csr_kernel",
    "spmm_rows_kernel" or None (a hub-only launch); hub_ms None without hub
    rows."""
    import ctypes
    lib = _lib.load()
    light = (ctypes.c_float * capacity)()
    hub = (ctypes.c_float * capacity)()
    span = (ctypes.c_float * capacity)()
    kind = (ctypes.c_int32 * capacity)()
    n = _lib._i64(0)
    _lib.check(lib.sgc_timing_collect_ex(*(ctypes.cast(b, ctypes.c_void_p)
                                           for b in (light, hub, span, kind)),
                                         capacity, ctypes_byref(n)), "timing_collect_ex")
    names = {0: "spmm_csr_kernel", 1: "spmm_rows_kernel", 2: "spmm_rows_kernel+hub (fused)",
             3: "spmm_csr_kernel+hub (fused)"}
    k = int(n.value)
    return ([float(light[i]) for i in range(k)],
            [float(hub[i]) if hub[i] >= 0 else None for i in range(k)],
            [float(span[i]) for i in range(k)],
            [names.get(int(kind[i])) for i in range(k)])


def _even_pitch_x16(X):
    """A 16-bit X in a layout the x16 classifier kernels take: unit column
    stride, even element pitch, 4-B aligned base -- X itself when it already
    is, else one copy into an even-pitch buffer (an odd K such as Cora's 1433
    or Citeseer's 3703 in a contiguous tensor, or a view that starts on an odd
    element)."""
    M, K = X.shape
    if X.stride(1) == 1 and X.stride(0) >= K and X.stride(0) % 2 == 0 and X.data_ptr() % 4 == 0:
        return X
    buf = torch.empty((M, K + (K & 1)), dtype=X.dtype, device=X.device)
    buf[:, :K].copy_(X)
    return buf[:, :K]


def _linear_x16(X, W, b, out):
    """The 16-bit-feature forward, or None where sgc_linear_x16 does not cover
    the shape (the caller upcasts)."""
    lib = _lib.load()
    M, K = X.shape
    C = W.shape[0]
    dt = X16_DTYPES[X.dtype]

    def named(t):
        return lib.sgc_linear_x16_kernel_name(M, K, t.stride(0), C, _lib.ptr(t), dt) != b"none"

    if M == 0:
        return out
    if not (X.stride(1) == 1 and X.stride(0) >= K and named(X)):
        X = _even_pitch_x16(X)  # a layout problem alone: one copy
        if not named(X):
            return None
    if M * out.stride(0) * 4 >= 2 ** 31:
        return None
    with torch.cuda.device(X.device):
        _lib.check(lib.sgc_linear_x16(_lib.ptr(X), dt, X.stride(0), _lib.ptr(W), _lib.ptr(b),
                                      _lib.ptr(out), out.stride(0), M, K, C,
                                      _lib.stream_handle(X.device)), "linear_x16")
    return out


def linear(X: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, out=None):
    """Y = X . W^T + b on MFMA (reference models.py:17-18, nn.Linear); W, b and
    Y (``out``) are float32.

    float32 X runs sgc_linear_f32.  torch.bfloat16 / torch.float16 X gives
    Y = float(X) . W^T + b on the exactly widened elements (nothing is rounded
    to 16 bits):
    * where sgc_linear_x16_kernel_name names a kernel for X as it lies in
      memory, sgc_linear_x16 reads the 16-bit rows directly;
    * a layout problem alone -- an odd element pitch or a 2-B-aligned base,
      e.g. a contiguous [N, 1433] or [N, 3703] tensor -- is fixed by one copy
      into an even-pitch 16-bit buffer, then the same kernel;
    * a shape the kernel does not cover (a class block whose W image exceeds
      LDS, e.g. K = 602 with 49 classes; offsets past 31 bits) takes
      X.float() and the float32 path.
    A non-finite x inside the K range gives non-finite logits in its row, not
    necessarily torch's +-inf."""
    _require_device(X, "input")
    if weight.dtype != torch.float32 or not (X.dtype == torch.float32 or is_x16(X)):
        raise TypeError("sgc_amd.linear: float32, bfloat16 or float16 features and float32 "
                        "weights only")
    if X.dim() != 2:
        raise ValueError("sgc_amd.linear: 2-D input expected")
    M, K = X.shape
    C = weight.shape[0]
    if weight.shape[1] != K:
        raise RuntimeError(f"sgc_amd.linear: shape mismatch {tuple(X.shape)} x {tuple(weight.shape)}^T")
    W = weight.contiguous()
    b = bias.contiguous() if bias is not None else None
    if out is None:
        out = torch.empty((M, C), dtype=torch.float32, device=X.device)
    if is_x16(X):
        if out.dtype != torch.float32:
            raise TypeError("sgc_amd.linear: out must be float32")
        if _linear_x16(X, W, b, out) is not None:
            return out
        X = X.float()  # not covered: the float32 kernels on the widened copy
    if X.stride(1) != 1 or X.stride(0) < K:
        X = X.contiguous()
    lib = _lib.load()
    with torch.cuda.device(X.device):
        _lib.check(lib.sgc_linear_f32(_lib.ptr(X), X.stride(0), _lib.ptr(W), _lib.ptr(b),
                                      _lib.ptr(out), out.stride(0), M, K, C,
                                      _lib.stream_handle(X.device)), "linear_f32")
    return out


def linear_backward(X: torch.Tensor, grad_out: torch.Tensor, want_bias=True):
    """(dW, db) of Y = X W^T + b for dY = grad_out: dW = dY^T X, db = sum_m dY
    (None unless want_bias), one read of X on MFMA.  At most 64 classes; dY, dW
    and db are float32.

    float32 X runs sgc_linear_backward_f32.  torch.bfloat16 / torch.float16 X
    gives dW = dY^T . float(X) on the exactly widened elements:
    * up to 48 classes sgc_linear_backward_x16 reads the 16-bit rows directly
      where sgc_linear_backward_x16_kernel_name names a kernel;
    * a layout problem alone (odd element pitch, 2-B-aligned base) is fixed by
      one copy into an even-pitch 16-bit buffer, then the same kernel;
    * above 48 classes, or past 31-bit offsets, it takes X.float() and the
      float32 path.
    A non-finite x gives a non-finite column of dW, not necessarily torch's
    +-inf."""
    _require_device(X, "input")
    M, K = X.shape
    C = grad_out.shape[1]
    if (grad_out.shape[0] != M or not (X.dtype == torch.float32 or is_x16(X)) or
            grad_out.dtype != torch.float32):
        raise RuntimeError("sgc_amd.linear_backward: shape/dtype mismatch")
    if C > 64:
        raise ValueError("sgc_amd.linear_backward: at most 64 classes")
    if grad_out.stride(1) != 1 or grad_out.stride(0) < C:
        grad_out = grad_out.contiguous()
    dW = torch.empty((C, K), dtype=torch.float32, device=X.device)
    db = torch.empty(C, dtype=torch.float32, device=X.device) if want_bias else None
    if M == 0:
        dW.zero_()
        if db is not None:
            db.zero_()
        return dW, db
    lib = _lib.load()
    if is_x16(X):
        dt = X16_DTYPES[X.dtype]

        def named(t):
            return lib.sgc_linear_backward_x16_kernel_name(M, K, t.stride(0), C, _lib.ptr(t),
                                                           dt) != b"none"

        X16 = X
        if not (X16.stride(1) == 1 and X16.stride(0) >= K and named(X16)):
            X16 = _even_pitch_x16(X16) if C <= 48 else None
        if X16 is not None and named(X16) and 32 * grad_out.stride(0) * 4 < 2 ** 31:
            ws_bytes = lib.sgc_linear_backward_x16_workspace(M, K, C)
            ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=X.device)
            with torch.cuda.device(X.device):
                _lib.check(lib.sgc_linear_backward_x16(
                    _lib.ptr(X16), dt, X16.stride(0), _lib.ptr(grad_out), grad_out.stride(0), M, K,
                    C, _lib.ptr(dW), _lib.ptr(db), _lib.ptr(ws), ws_bytes,
                    _lib.stream_handle(X.device)), "linear_backward_x16")
            return dW, db
        X = X.float()  # not covered: the float32 kernels on the widened copy
    if X.stride(1) != 1 or X.stride(0) < K:
        X = X.contiguous()
    ws_bytes = lib.sgc_linear_backward_workspace(M, K, C)
    ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(lib.sgc_linear_backward_f32(_lib.ptr(X), X.stride(0), _lib.ptr(grad_out),
                                               grad_out.stride(0), M, K, C, _lib.ptr(dW),
                                               _lib.ptr(db), _lib.ptr(ws), ws_bytes,
                                               _lib.stream_handle(X.device)), "linear_backward_f32")
    return dW, db


def xent_x16_layout(X, C, copy=True):
    """A 16-bit X as the fused 16-bit step (sgc_linear_xent_x16) takes it, or
    None where sgc_linear_xent_x16_kernel_name does not cover it: X itself
    where it is covered as it lies in memory; with `copy`, a layout problem
    alone (odd element pitch, 2-B-aligned base) is fixed by one
    _even_pitch_x16 copy, the rule `linear` follows."""
    lib = _lib.load()
    M, K = X.shape
    dt = X16_DTYPES[X.dtype]

    def named(t):
        return lib.sgc_linear_xent_x16_kernel_name(M, K, t.stride(0), C, _lib.ptr(t),
                                                   dt) != b"none"

    if M == 0:
        return None
    if X.stride(1) == 1 and X.stride(0) >= K and named(X):
        return X
    if not copy or C > 48:
        return None
    X = _even_pitch_x16(X)
    return X if named(X) else None


def linear_xent(X: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                labels: torch.Tensor, want_logits=False):
    """Fused SGC training step: (loss, dW, db[, logits]) for
    F.cross_entropy(X W^T + b, labels) (mean), on the GPU; everything returned
    is float32.

    float32 X runs sgc_linear_xent_f32.  torch.bfloat16 / torch.float16 X gives
    the step on the exactly widened elements, X read twice at 16 bits
    (sgc_linear_xent_x16), where sgc_linear_xent_x16_kernel_name covers it --
    after one even-pitch copy where the layout alone is the problem (an odd
    pitch such as 1433 or 3703, a 2-B-aligned base); anything still uncovered
    (more than 48 classes, W's image past LDS, offsets past 31 bits) takes
    X.float() and the float32 step.  want_logits on 16-bit X takes the logits
    from `linear` (the fused 16-bit step forms none)."""
    _require_device(X, "input")
    if not (X.dtype == torch.float32 or is_x16(X)) or weight.dtype != torch.float32:
        raise TypeError("sgc_amd.linear_xent: float32, bfloat16 or float16 features and float32 "
                        "weights only")
    M, K = X.shape
    C = weight.shape[0]
    if weight.shape[1] != K or labels.shape != (M,):
        raise RuntimeError("sgc_amd.linear_xent: shape mismatch")
    if C > 64:
        raise ValueError("sgc_amd.linear_xent: at most 64 classes")
    if X.stride(1) != 1 or X.stride(0) < K:
        X = X.contiguous()
    W = weight.detach().contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    y = labels.to(device=X.device, dtype=torch.int64).contiguous()
    if M:
        # F.cross_entropy raises on a label outside [0, C) (and skips
        # ignore_index=-100 rows, which the fused kernel does not support):
        # refuse loudly instead of returning a silently different loss
        lo, hi = (int(v) for v in torch.aminmax(y))
        if lo < 0 or hi >= C:
            raise ValueError(f"sgc_amd.linear_xent: labels must lie in [0, {C}), got "
                             f"[{lo}, {hi}] (ignore_index is not supported)")
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=X.device)
    dW = torch.empty_like(W)
    db = torch.empty(C, dtype=torch.float32, device=X.device) if b is not None else None
    if is_x16(X):
        X16 = xent_x16_layout(X, C)
        if X16 is not None:
            ws_bytes = lib.sgc_linear_xent_x16_workspace(M, K, C)
            ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=X.device)
            with torch.cuda.device(X.device):
                _lib.check(lib.sgc_linear_xent_x16(
                    _lib.ptr(X16), X16_DTYPES[X16.dtype], X16.stride(0), _lib.ptr(W), _lib.ptr(b),
                    _lib.ptr(y), M, K, C, _lib.ptr(loss), _lib.ptr(dW), _lib.ptr(db), _lib.ptr(ws),
                    ws_bytes, _lib.stream_handle(X.device)), "linear_xent_x16")
            return (loss, dW, db, linear(X16, W, b)) if want_logits else (loss, dW, db)
        X = X.float()  # not covered: the float32 step on the widened copy
    logits = torch.empty((M, C), dtype=torch.float32, device=X.device) if want_logits else None
    ws_bytes = lib.sgc_linear_xent_workspace(M, K, C)
    ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(lib.sgc_linear_xent_f32(_lib.ptr(X), X.stride(0), _lib.ptr(W), _lib.ptr(b),
                                           _lib.ptr(y), M, K, C, _lib.ptr(loss), _lib.ptr(dW),
                                           _lib.ptr(db), _lib.ptr(logits), C, _lib.ptr(ws),
                                           ws_bytes, _lib.stream_handle(X.device)),
                   "linear_xent_f32")
    return (loss, dW, db, logits) if want_logits else (loss, dW, db)


class LinearEval(NamedTuple):
    """What `linear_eval` leaves on X's device (None where not asked for)."""
    pred: torch.Tensor                  # int64 [M]
    confusion: Optional[torch.Tensor]   # int64 [C, C], row = label, column = prediction
    counts: Optional[torch.Tensor]      # int64 [2]: rows counted, rows correct
    loss: Optional[torch.Tensor]        # float32 0-d, mean cross-entropy


def _eval_from_logits(logits, labels):
    """`linear_eval`'s outputs from a logits matrix with torch ops: the path of
    CPU tensors and of shapes the evaluation kernels do not cover."""
    C = logits.shape[1]
    pred = logits.max(1)[1]
    if labels is None:
        return LinearEval(pred, None, None, None)
    ok = (labels >= 0) & (labels < C)
    y, p = labels[ok], pred[ok]
    confusion = torch.bincount(y * C + p, minlength=C * C).reshape(C, C)
    counts = torch.stack([ok.sum(), (p == y).sum()]).to(torch.int64)
    if bool(ok.all()):
        loss = _nnf.cross_entropy(logits.float(), labels) if len(labels) else logits.new_zeros(())
    else:  # a label outside [0, C): the kernels' NaN
        loss = logits.new_full((), float("nan"), dtype=torch.float32)
    return LinearEval(pred, confusion, counts, loss.detach())


def linear_eval(X: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None):
    """Evaluate the classifier z = X . W^T + b without forming z: a LinearEval
    of the predictions (torch's z.max(1)[1]) and, with `labels`, the confusion
    matrix (row = label, column = prediction), {rows counted, rows correct} and
    the mean cross-entropy -- all left on X's device (the kernel path never
    synchronises with the host; the torch-op path reads one flag back).

    float32 X runs sgc_linear_eval_f32; torch.bfloat16 / torch.float16 X runs
    sgc_linear_eval_x16 on the exactly widened elements where
    sgc_linear_eval_x16_kernel_name covers it, after one even-pitch copy where
    the layout alone is the problem (`linear`'s rule).  Anything still
    uncovered (more than 64 classes, W's image past LDS, offsets past 31 bits)
    takes the logits from `linear` and forms the same outputs with torch ops
    (max, bincount, F.cross_entropy); CPU tensors take the torch ops as well.
    A label outside [0, C) leaves its row out of the matrix and the counts and
    makes the loss NaN."""
    if weight.dtype != torch.float32 or not (X.dtype == torch.float32 or is_x16(X)):
        raise TypeError("sgc_amd.linear_eval: float32, bfloat16 or float16 features and float32 "
                        "weights only")
    if X.dim() != 2:
        raise ValueError("sgc_amd.linear_eval: 2-D input expected")
    M, K = X.shape
    C = weight.shape[0]
    if weight.shape[1] != K or (labels is not None and labels.shape != (M,)):
        raise RuntimeError("sgc_amd.linear_eval: shape mismatch")
    W = weight.detach().contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    y = None
    if labels is not None:
        y = labels.to(device=X.device, dtype=torch.int64).contiguous()
    if X.device.type == "cpu":
        return _eval_from_logits(_nnf.linear(X.float(), W, b), y)
    lib = _lib.load()
    call = None
    if M and is_x16(X):
        dt = X16_DTYPES[X.dtype]

        def named(t):
            return lib.sgc_linear_eval_x16_kernel_name(M, K, t.stride(0), C, _lib.ptr(t),
                                                       dt) != b"none"

        X16 = X
        if not (X16.stride(1) == 1 and X16.stride(0) >= K and named(X16)):
            X16 = _even_pitch_x16(X16) if C <= 64 else None  # a layout problem alone: one copy
        if X16 is not None and named(X16):
            ws_bytes = lib.sgc_linear_eval_x16_workspace(M, K, C)

            def call(*out):
                return lib.sgc_linear_eval_x16(_lib.ptr(X16), dt, X16.stride(0), *out)
    elif M:
        Xc = X if X.stride(1) == 1 and X.stride(0) >= K else X.contiguous()
        if lib.sgc_linear_eval_kernel_name(M, K, Xc.stride(0), C, _lib.ptr(Xc)) != b"none":
            ws_bytes = lib.sgc_linear_eval_workspace(M, K, C)

            def call(*out):
                return lib.sgc_linear_eval_f32(_lib.ptr(Xc), Xc.stride(0), *out)
    if call is None:  # not covered (or empty): the logits, then torch ops
        return _eval_from_logits(linear(X, W, b), y)
    dev = X.device
    pred = torch.empty(M, dtype=torch.int64, device=dev)
    confusion = counts = loss = None
    if y is not None:
        confusion = torch.empty((C, C), dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
    ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(call(_lib.ptr(W), _lib.ptr(b), _lib.ptr(y), M, K, C, _lib.ptr(pred),
                        _lib.ptr(confusion), _lib.ptr(counts), _lib.ptr(loss), _lib.ptr(ws),
                        ws_bytes, _lib.stream_handle(dev)), "linear_eval")
    return LinearEval(pred, confusion, counts, loss)
