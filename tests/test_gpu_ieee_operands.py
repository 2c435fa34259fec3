"""The SpMM kernels on operands that reach every IEEE edge (tests/ieee_operands.py).

The rest of the GPU suite runs aug-normalised S in (0, 1] against randn X:
every intermediate of a chain is a normal number, and a kernel that runs one
FMA too many with a zero weight, flushes subnormals or takes the first product
by a multiply returns the same bits there.  Here S has both signs, zeros and
subnormals, X has subnormal, huge, infinite and NaN elements, and the rows
have every length at which a kernel body changes: 0..5, 8, 15..17, 31..33, 40,
63..65, 100 nonzeros, long rows of 300 / 900 / 3001 that meet inf and NaN only
at their first and last nonzero and either side of a 64-, 240- and
480-nonzero boundary, and all-negative rows whose chains end in -0.0.

Rule (ieee_operands.compare): NaN exactly where the reference has NaN, payload
and sign free; every other element bit-equal.  Reference: the oracle, which
tests/test_ieee_operands_cpu.py shows equal to torch.spmm on these operands.

Which kernel body a case reaches is the choice of spmm_schedule()
(csrc/spmm_schedule.h), which launch_spmm launches as returned:
tests/test_spmm_schedule_host.py asks sgc_spmm_kernel_name for these
parametrisations and asserts the bodies the docstrings below name (and the
wide items count their launches; that counter is asserted here).
Every knob is restored in `finally`.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import ieee_operands as io

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 4096
WIDTHS = [1, 3, 12, 33, 64, 65, 130, 152, 256, 602]
# default plan; every row a hub; every row heavy; heavy + hub mixes; light only
SCHEDULES = [(None, None), (0, 0), (0, 10**9), (16, 200), (40, 500), (10**9, 10**9)]
KNOB_DEFAULTS = {"rows_per_wave": 0, "heavy_pairs": 29, "hub_chunk": 0, "hub_loaders": 15,
                 "hub_stream": 0, "hub_fuse": 1, "short_wide": -1, "short_wide_first": 0,
                 "max_vec": 4, "x16_vec": 0}


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgc_amd import _lib
    _lib.load()
    for k, v in KNOB_DEFAULTS.items():
        assert _get(k) == v, f"{k} is not at its default"


def _get(key):
    from sgc_amd import _lib
    return int(_lib.load().sgc_get_tuning(key.encode()))


class knobs:
    """with knobs(rows_per_wave=2, ...): set, and back to the defaults after."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from sgc_amd import _lib
        lib = _lib.load()
        for k, v in self.kw.items():
            _lib.check(lib.sgc_set_tuning(k.encode(), int(v)), f"set_tuning {k}")

    def __exit__(self, *exc):
        from sgc_amd import _lib
        lib = _lib.load()
        for k in self.kw:
            lib.sgc_set_tuning(k.encode(), KNOB_DEFAULTS[k])


def _kw(th, hub):
    return {} if th is None else {"threshold": th, "hub_threshold": hub}


@functools.lru_cache(maxsize=None)
def device_csr(kind="wild"):
    from sgc_amd.propagate import DeviceCSR
    g = io.edge_graph(N, 0, kind)
    return DeviceCSR.from_host_arrays(g.row_ptr, g.col_idx, g.val, device=DEV)


@functools.lru_cache(maxsize=None)
def reference(kind, F, K=1):
    """(oracle result on the host, the same on the device); never written to."""
    from oracle import oracle as o
    o.build()
    g = io.edge_graph(N, 0, kind)
    want = o.propagate(g.row_ptr, g.col_idx, g.val, io.edge_features(N, F, kind), K)
    want.setflags(write=False)
    return want, torch.from_numpy(want.copy()).to(DEV)


def _bad(got, want_dev):
    gn, wn = torch.isnan(got), torch.isnan(want_dev)
    if got.dtype == torch.float32:
        gb, wb = got.contiguous().view(torch.int32), want_dev.contiguous().view(torch.int32)
    else:
        gb, wb = got.contiguous().view(torch.int16), want_dev.contiguous().view(torch.int16)
    return (gn != wn) | (~wn & (gb != wb))


def check(got, want, want_dev, what):
    """The rule, evaluated on the device; the host comparison words the failure."""
    torch.cuda.synchronize()
    assert got.shape == want_dev.shape, (what, got.shape, want_dev.shape)
    if bool(_bad(got, want_dev).any()):
        io.compare(got.cpu() if got.dtype != torch.float32 else got.cpu().numpy(), want, str(what))
        raise AssertionError(f"{what}: device and host comparison disagree")


class Layout:
    """X and out for one launch.  "lines": 128-B rows, both flagged padded (the
    engine's own buffers: 16-B lanes at any F); "contig": exactly [n, F];
    "slice": columns 3..3+F of an F + 7 wide tensor (no alignment, 4-B lanes).
    Everything outside the F columns is NaN: X's padding must not reach a
    result, out's must stay NaN (flagged padded: from round4(F) on)."""

    def __init__(self, how, F, dtype=torch.float32):
        from sgc_amd.propagate import SPMM_X_PADDED, SPMM_Y_PADDED
        self.how, self.F, self.dtype = how, F, dtype
        per_line = 32 if dtype == torch.float32 else 64
        if how == "lines":
            self.ld, self.off = (F + per_line - 1) // per_line * per_line + per_line, 0
            self.flags = (SPMM_X_PADDED | SPMM_Y_PADDED) if dtype == torch.float32 else 0
            self.free = (F + 3) // 4 * 4 if dtype == torch.float32 else F
        elif how == "contig":
            self.ld, self.off, self.flags, self.free = F, 0, 0, F
        else:
            self.ld, self.off, self.flags, self.free = F + 7, 3, 0, F

    def x(self, X):
        buf = torch.full((X.shape[0], self.ld), float("nan"), dtype=self.dtype, device=DEV)
        view = buf[:, self.off:self.off + self.F]
        view.copy_(X if isinstance(X, torch.Tensor) else torch.from_numpy(X.copy()))
        return view

    def out(self, rows, dtype=None):
        buf = torch.full((rows, self.ld), float("nan"), dtype=dtype or self.dtype, device=DEV)
        return buf, buf[:, self.off:self.off + self.F]

    def padding_untouched(self, buf):
        return bool(torch.isnan(buf[:, :self.off]).all() and
                    torch.isnan(buf[:, self.off + self.free:]).all())


def v4_ok(F, how):
    """launch_spmm's v4_ok: 16-B lanes possible (then rows_per_wave matters)."""
    F4 = (F + 3) // 4 * 4
    return F4 >= 32 and (how == "lines" or (how == "contig" and F % 4 == 0))


def _one_hop(F, how, schedules=SCHEDULES, use_plan=True, rows=(0, N), kind="wild", what=()):
    from sgc_amd.propagate import spmm
    want, want_dev = reference(kind, F)
    lay = Layout(how, F)
    Xd = lay.x(io.edge_features(N, F, kind))
    r0, r1 = rows
    for th, hub in schedules:
        buf, out = lay.out(r1 - r0)
        spmm(device_csr(kind), Xd, r0, r1, out=out, flags=lay.flags, use_plan=use_plan,
             **_kw(th, hub))
        check(out, want[r0:r1], want_dev[r0:r1], (F, how, th, hub, rows) + tuple(what))
        assert lay.padding_untouched(buf), (F, how, th, hub, "padding written")


# ---- one hop, "wild" ------------------------------------------------------------

ONE_HOP = [(F, how, rpw) for F in WIDTHS for how in ("lines", "contig", "slice")
           for rpw in ((0, 1, 2, 4) if v4_ok(F, how) else (0,))]


@pytest.mark.parametrize("F,how,rows_per_wave", ONE_HOP)
def test_one_hop_every_schedule(F, how, rows_per_wave):
    """spmm() under the six schedules.  Light rows: without 16-B lanes (F4 < 32,
    "slice", "contig" at F % 4 != 0) spmm_csr_kernel's row_chunks_pipe with 1-
    or 2-float lanes (4-float at 12 floats in aligned rows: the one-row kernel's
    own lanes), where rows_per_wave changes nothing and only 0 runs;
    with them spmm_rows_kernel's LDS blocks (rows_per_wave 2 / 4, or 0 below
    128 floats and at F % 4 != 0: 9..32 lanes per row, 1..5 slices, 10 at 602
    floats and 16 lanes) or the one-row kernel (rows_per_wave 1: 16-B lanes at
    F % 4 == 0 and at 130 padded floats, else 1- or 2-float lanes; 0: 16-B
    lanes at 130 / 152 / 256 and, as the small-wide rule's 512-float slices of
    2-float lanes, at 602).  Heavy rows (threshold
    0 / 16 / 40): row_pairs_pipe, row_quadsT_pipe at 33..64 floats, row_chunks_pipe
    sub-chunks.  Hub rows (0 / 200 / 500 and the default plan's 3001-nonzero
    rows): hub_body with hub_chain_dpp rounds and the scalar tail, fused into
    the light launch where the dispatch allows (serial hubs of <= 3072
    nonzeros), else spmm_hub_kernel; (0, 0) sends rows of 1..100 nonzeros
    through the hub body too."""
    with knobs(rows_per_wave=rows_per_wave):
        _one_hop(F, how, what=(rows_per_wave,))


@pytest.mark.parametrize("heavy_pairs", [0, 1, 5, 13, 17, 29, 31])
@pytest.mark.parametrize("F,how,rows_per_wave", [(30, "lines", 0), (32, "contig", 0),
                                                 (33, "lines", 0), (64, "contig", 0),
                                                 (65, "lines", 0), (130, "lines", 2),
                                                 (602, "lines", 2), (152, "contig", 1),
                                                 (256, "lines", 0), (3, "slice", 0)])
def test_heavy_row_bodies(F, how, rows_per_wave, heavy_pairs):
    """heavy_pairs at the widths each bit applies to: bit 4 row_quads_pipe at
    32 computed floats, the only width of at most 32 the multi-row kernel
    takes (30 in padded rows, 32; not among the one-hop widths); bit 8
    row_quadsT_pipe at 33..64 floats (33, 64), without it the pairs; bit 1
    row_pairs_pipe (one item per row and slice) against sub-chunk
    row_chunks_pipe items, bit 16 its transposed form (65, 130, 602 on the
    multi-row kernel); bit 2 row_pairs_pipe inside spmm_csr_kernel's 16-B-lane
    heavy items (152, 256); at 3 floats no bit applies (4-B lanes)."""
    with knobs(rows_per_wave=rows_per_wave, heavy_pairs=heavy_pairs):
        _one_hop(F, how, [(0, 10**9), (16, 200), (40, 500)], what=(heavy_pairs,))


@pytest.mark.parametrize("hub_chunk", [0, 32, 64])
@pytest.mark.parametrize("F,how", [(64, "lines"), (130, "lines"), (152, "lines"), (65, "slice"),
                                   (602, "lines")])
def test_hub_kernel_knobs(F, how, hub_chunk):
    """hub_loaders {15, 7} x hub_stream {0, 1, 2} x hub_fuse {0, 1} per hub_chunk:
    spmm_hub_kernel<32 | 64, 15 | 7> beside the light kernel (1) or before it
    (2, and 0 here: the longest hub has 3001 <= 3072 nonzeros), and with
    hub_chunk 0 and hub_fuse 1 the hub items inside the light launch (hub_body
    from spmm_rows_kernel / spmm_csr_kernel).  128-B rows ("lines") take
    32-float chunks by default up to 192 floats; the unaligned slice 64."""
    for loaders in (15, 7):
        for stream in (0, 1, 2):
            for fuse in (0, 1):
                with knobs(hub_chunk=hub_chunk, hub_loaders=loaders, hub_stream=stream,
                           hub_fuse=fuse):
                    _one_hop(F, how, [(0, 0), (16, 200), (40, 500)],
                             what=(hub_chunk, loaders, stream, fuse))


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("ts", [0, 4, 16, 32])
@pytest.mark.parametrize("F,how", [(130, "lines"), (152, "contig"), (256, "lines"), (602, "lines")])
def test_wide_items(F, how, ts, first):
    """short_wide Ts: light rows of at most Ts nonzeros cross every slice in one
    wave (wide_rows_body<16> up to 16, <32> above), their workgroups before or
    after the slices'.  Needs the multi-row kernel at 32 lanes per row over at
    least two slices (rows_per_wave 2) and no fused hub rows (hub_fuse 0).  The
    launches that took wide items are counted by the library."""
    with knobs(rows_per_wave=2, hub_fuse=0, short_wide=ts, short_wide_first=first):
        before = _get("short_wide_launches")
        _one_hop(F, how, [(None, None), (40, 500), (10**9, 10**9)], what=(ts, first))
        assert _get("short_wide_launches") - before == (3 if ts else 0)


@pytest.mark.parametrize("max_vec", [1, 2, 4])
@pytest.mark.parametrize("F,how,rows_per_wave", [(12, "contig", 0), (130, "lines", 1),
                                                 (130, "contig", 0), (152, "contig", 1),
                                                 (256, "contig", 0), (602, "contig", 0)])
def test_lane_width_of_the_one_row_kernel(F, how, rows_per_wave, max_vec):
    """max_vec caps spmm_csr_kernel's lanes: row_chunks_pipe<1 | 2 | 4, C> with
    1..8 chunks per lane on the same rows."""
    with knobs(rows_per_wave=rows_per_wave, max_vec=max_vec):
        _one_hop(F, how, [(None, None), (16, 200), (10**9, 10**9)], what=(max_vec,))


@pytest.mark.parametrize("F", WIDTHS)
def test_no_plan(F):
    """use_plan=False: every row, the 3001-nonzero ones too, is a light item of
    the launch's light kernel (LDS blocks refilled ~190 times / row_chunks_pipe's
    main loop and tail)."""
    for how in ("lines", "slice"):
        _one_hop(F, how, [(None, None)], use_plan=False)


@pytest.mark.parametrize("rows", [(5, 2300), (586, 587), (1405, 1406), (4000, N), (0, 1)])
@pytest.mark.parametrize("F,how", [(33, "lines"), (130, "lines"), (602, "lines"), (65, "slice")])
def test_row_ranges(F, how, rows):
    """A partial row range: (586, 587) is the 3001-nonzero row alone, (1405,
    1406) the long all-negative one, (0, 1) an empty row."""
    g = io.edge_graph(N)
    assert np.diff(g.row_ptr)[586] == 3001 and 1405 in g.negative_rows
    for rpw in (0, 2) if v4_ok(F, how) else (0,):
        with knobs(rows_per_wave=rpw):
            _one_hop(F, how, [(None, None), (16, 200), (10**9, 10**9)], rows=rows, what=(rpw,))


def test_gfx950_nan_patterns_information():
    """Printed only (run with -s): the NaN bit patterns the kernels return next
    to the oracle's on the host; the rule compares neither payload nor sign."""
    from sgc_amd.propagate import spmm
    want, _ = reference("wild", 130)
    got = spmm(device_csr(), torch.from_numpy(io.edge_features(N, 130, "wild").copy()).to(DEV))
    got = got.cpu().numpy()
    print("NaN patterns: gfx950", io.nan_patterns(got), "host oracle", io.nan_patterns(want))
    io.compare(got, want, "F=130")


# ---- accumulate and column groups, "wild" -----------------------------------------

@pytest.mark.parametrize("rows_per_wave", [0, 1, 2])
@pytest.mark.parametrize("F,how", [(3, "slice"), (33, "lines"), (130, "lines"), (256, "contig"),
                                   (602, "lines")])
def test_accumulate_over_column_splits(F, how, rows_per_wave):
    """SPMM_ACCUMULATE: block 0 plain into a NaN-filled out, the other blocks
    continue the stored chains -- from a stored -0.0 (which only survives if
    no FMA is added for a row without nonzeros in the block), inf or NaN.
    [0, 5, n] leaves block 0 nearly empty: most rows start from a written +0.0."""
    from sgc_amd.propagate import SPMM_ACCUMULATE, DeviceCSR, spmm
    if rows_per_wave and not v4_ok(F, how):
        rows_per_wave = 0
    g = io.edge_graph(N)
    want, want_dev = reference("wild", F)
    lay = Layout(how, F)
    Xd = lay.x(io.edge_features(N, F, "wild"))
    with knobs(rows_per_wave=rows_per_wave):
        for bounds in ([0, 700, 1100, 1600, N], [0, 5, N]):
            subs = [DeviceCSR.from_host_arrays(*t, n_cols=N, device=DEV)
                    for t in io.column_groups(g, bounds)]
            for th, hub in ((None, None), (40, 500), (10**9, 10**9)):
                for r0, r1 in ((0, N), (5, 2300)):
                    buf, out = lay.out(r1 - r0)
                    for i, sub in enumerate(subs):
                        spmm(sub, Xd, r0, r1, out=out, **_kw(th, hub),
                             flags=lay.flags | (SPMM_ACCUMULATE if i else 0))
                    check(out, want[r0:r1], want_dev[r0:r1], (F, how, bounds, th, hub, r0, r1))
                    assert lay.padding_untouched(buf)


@pytest.mark.parametrize("whole_rows", [0, 32])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("F", [130, 602])
def test_column_groups(F, G, whole_rows):
    """The device's own column split (sgc_csr_colsplit_ex), rows of at most
    `whole_rows` nonzeros kept whole in group 0 and skipped by the accumulate
    launches, through propagate()'s K = 1 loop and through spmm() per group."""
    from sgc_amd.propagate import SPMM_ACCUMULATE, propagate, spmm
    mod = importlib.import_module("sgc_amd.propagate")
    csr = device_csr()
    want, want_dev = reference("wild", F)
    X = torch.from_numpy(io.edge_features(N, F, "wild").copy()).to(DEV)
    saved = mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS
    try:
        mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS = G, whole_rows
        for rpw in (0, 2):
            with knobs(rows_per_wave=rpw):
                out = propagate(csr, X, 1, threshold=40, hub_threshold=500, prepare=False)
                check(out, want, want_dev, (F, G, whole_rows, rpw, "propagate"))
                mod.COLUMN_GROUPS = 1  # spmm() below launches the groups itself
                out = torch.full((N, F), float("nan"), device=DEV)
                for i, part in enumerate(csr.column_groups(G, whole_rows)):
                    spmm(part, X, out=out, flags=SPMM_ACCUMULATE if i else 0)
                check(out, want, want_dev, (F, G, whole_rows, rpw, "spmm"))
                mod.COLUMN_GROUPS = G
    finally:
        mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS = saved
        csr.drop_groups()


# ---- several hops, "quiet" ------------------------------------------------------------

@pytest.mark.parametrize("F", [65, 130])
def test_three_hops_every_loop(F):
    """K = 3 on the finite operands (subnormals and -0.0 feed hops 2 and 3):
    the Python loop (a hop_hook keeps it unrecorded), the native loop, the
    recorded launch list (second call replays) and the captured HIP graph."""
    from sgc_amd.propagate import GraphedPropagation, propagate
    csr = device_csr("quiet")
    want, want_dev = reference("quiet", F, 3)
    X = torch.from_numpy(io.edge_features(N, F, "quiet").copy()).to(DEV)
    try:
        for th, hub in ((None, None), (16, 200)):
            kw = _kw(th, hub)
            check(propagate(csr, X, 3, hop_hook=lambda *a: None, **kw), want, want_dev, "python")
            check(propagate(csr, X, 3, native_loop=True, **kw), want, want_dev, "native")
            for i in range(2):
                out = torch.full((N, F), float("nan"), device=DEV)
                check(propagate(csr, X, 3, out=out, **kw), want, want_dev, ("list", i))
            gp = GraphedPropagation(csr, (N, F), 3, **kw)
            check(gp.run(X), want, want_dev, "graph")
            check(gp.run(X), want, want_dev, "graph replay")
    finally:
        csr.release_prepared()


def test_sgc_precompute_shuffled_coo_with_duplicates(oracle):
    """The drop-in on the COO in shuffled storage order with duplicates: the
    ingest's sort keeps each row's storage order, which is the FMA order."""
    from sgc_amd.utils import sgc_precompute
    F = 65
    r, c, v = io.edge_coo(N, 0, "quiet")
    X = io.edge_features(N, F, "quiet")
    rp, ci, va = oracle.coo_to_csr(N, N, r, c, v)
    want = oracle.propagate(rp, ci, va, X, 3)
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([r, c])), torch.from_numpy(v),
                                  (N, N)).to(DEV)
    out, _ = sgc_precompute(torch.from_numpy(X.copy()).to(DEV), adj, 3)
    torch.cuda.synchronize()
    io.compare(out.cpu().numpy(), want, "sgc_precompute K=3")


@pytest.mark.parametrize("ndev", [2, 3])
def test_mgpu_engine_virtual_devices(ndev):
    """The native multi-device engine's feature blocks over virtual devices."""
    from sgc_amd.multigpu import DeviceSet
    F = 130
    want, want_dev = reference("quiet", F, 3)
    X = torch.from_numpy(io.edge_features(N, F, "quiet").copy()).to(DEV)
    out = torch.full((N, F), float("nan"), device=DEV)
    DeviceSet.get([0] * ndev).propagate(device_csr("quiet"), X, 3, out)
    check(out, want, want_dev, ("mgpu", ndev))


# ---- 16-bit features -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference16(kind, F, dtype, K=1, last_fp32=False):
    from oracle import oracle as o
    from test_gpu_x16 import emulate
    o.build()
    g = io.edge_graph(N, 0, kind)
    want = emulate(o, (g.row_ptr, g.col_idx, g.val), io.edge_features16(N, F, kind, dtype), K,
                   last_fp32)
    return want, want.to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("x16_vec", [0, 1, 8])
@pytest.mark.parametrize("F", [65, 130, 602])
def test_x16_one_hop_wild(F, x16_vec, dtype):
    """spmm16.hip on the operands at the 16-bit format's own exponents: 16-bit
    patterns against the emulation (fp32 chains on the widened elements, one
    rounding), lanes of 1 or 8 elements or the rule's, 128-B rows and an
    unaligned slice, light + heavy + hub rows and light rows only; and the
    unrounded fp32 output continued by an accumulate launch over a column
    split."""
    from sgc_amd.propagate import SPMM_ACCUMULATE, DeviceCSR, spmm
    g = io.edge_graph(N)
    X16 = io.edge_features16(N, F, "wild", dtype)
    want, want_dev = reference16("wild", F, dtype)
    want32, want32_dev = reference16("wild", F, dtype, 1, True)
    with knobs(x16_vec=x16_vec):
        for how in ("lines", "slice"):
            lay = Layout(how, F, dtype)
            Xd = lay.x(X16)
            for th, hub in ((40, 500), (10**9, 10**9)):
                buf, out = lay.out(N)
                spmm(device_csr(), Xd, out=out, **_kw(th, hub))
                check(out, want, want_dev, (F, x16_vec, dtype, how, th))
                assert lay.padding_untouched(buf)
            out = torch.full((N, F), float("nan"), device=DEV)
            for i, t in enumerate(io.column_groups(g, [0, 700, 1600, N])):
                sub = DeviceCSR.from_host_arrays(*t, n_cols=N, device=DEV)
                spmm(sub, Xd, out=out, threshold=40, hub_threshold=500,
                     out_dtype=torch.float32, flags=SPMM_ACCUMULATE if i else 0)
            check(out, want32.numpy(), want32_dev, (F, x16_vec, dtype, how, "fp32 accumulate"))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_x16_three_hops_quiet(dtype):
    from sgc_amd.propagate import propagate
    F = 130
    want, want_dev = reference16("quiet", F, dtype, 3)
    Xd = Layout("lines", F, dtype).x(io.edge_features16(N, F, "quiet", dtype))
    for th, hub in ((None, None), (16, 200)):
        check(propagate(device_csr("quiet"), Xd, 3, **_kw(th, hub)), want, want_dev, (dtype, th))


# ---- the million-row schedule ------------------------------------------------------

BIG = 1 << 20  # kChunksPipe2Rows: launches of at least this many rows take row_chunks_pipe2


@functools.lru_cache(maxsize=None)
def big_csr():
    from sgc_amd.propagate import DeviceCSR
    b = io.big_graph(BIG)
    return DeviceCSR.from_host_arrays(b.row_ptr, b.col_idx, b.val, device=DEV)


@functools.lru_cache(maxsize=None)
def big_reference(F):
    """(X, oracle result), both on the device only."""
    from oracle import oracle as o
    o.build()
    b = io.big_graph(BIG)
    X = io.edge_features(BIG, F, "wild")
    want = torch.from_numpy(o.spmm_csr(b.row_ptr, b.col_idx, b.val, X)).to(DEV)
    return torch.from_numpy(X).to(DEV), want


def _big_check(got, want, what):
    torch.cuda.synchronize()
    bad = _bad(got, want)
    n_bad = int(bad.sum())
    if n_bad:
        r, c = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"{what}: {n_bad} elements differ; first at ({r}, {c}): "
                             f"got {got[r, c].item()!r}, want {want[r, c].item()!r}")


@pytest.mark.parametrize("F", [5, 24, 130])
def test_million_row_schedule(F):
    """2^20 rows with rows_per_wave = 1: spmm_csr_kernel's whole-block schedule
    row_chunks_pipe2 (no knob selects it; only the row count does) with 1-, 4-
    and 2-float lanes (130 floats: two slices of one 128-float chunk) on rows
    of 0..8 nonzeros, 300 heavy rows of 65..300 and three of 3001 (default
    plan and (40, 500)), heavy_pairs 29 and 31, and in a caller's buffer with
    an odd leading dimension (4-B lanes; 130 floats: two chunks per lane).
    The same launch over rows [0, 2^20 - 1) stays on row_chunks_pipe: the
    control below the switch."""
    from sgc_amd.propagate import spmm
    csr = big_csr()
    X, want = big_reference(F)
    odd = torch.full((BIG, F + 3), float("nan"), device=DEV)
    odd[:, 1:1 + F] = X
    for hp in (29, 31):
        with knobs(rows_per_wave=1, heavy_pairs=hp):
            for th, hub in ((None, None), (40, 500)):
                _big_check(spmm(csr, X, **_kw(th, hub)), want, (F, hp, th, "2^20"))
                _big_check(spmm(csr, X, 0, BIG - 1, **_kw(th, hub)), want[:BIG - 1],
                           (F, hp, th, "2^20 - 1"))
            out = torch.full((BIG, F + 3), float("nan"), device=DEV)
            spmm(csr, odd[:, 1:1 + F], out=out[:, 1:1 + F])
            _big_check(out[:, 1:1 + F], want, (F, hp, "odd leading dimension"))
            assert bool(torch.isnan(out[:, 0]).all() and torch.isnan(out[:, 1 + F:]).all())


def test_million_row_accumulate():
    """One SPMM_ACCUMULATE pass over two column blocks at 24 floats, out
    starting as NaN: row_chunks_pipe2 continuing stored chains."""
    from sgc_amd.propagate import SPMM_ACCUMULATE, DeviceCSR, spmm
    F = 24
    X, want = big_reference(F)
    b = io.big_graph(BIG)
    out = torch.full((BIG, F), float("nan"), device=DEV)
    with knobs(rows_per_wave=1):
        for i, t in enumerate(io.column_groups(b, [0, BIG // 3, BIG])):
            sub = DeviceCSR.from_host_arrays(*t, n_cols=BIG, device=DEV)
            spmm(sub, X, out=out, threshold=40, hub_threshold=500,
                 flags=SPMM_ACCUMULATE if i else 0)
    _big_check(out, want, "accumulate")
