"""Wide items of the multi-row SpMM kernel (the "short_wide" knob,
sgc_spmm_csr_f32_ex3): a light row of at most Ts nonzeros crosses every feature
slice in one wave.  It is a schedule only, so everything here is compared with
torch.equal / bit patterns against the library's CPU twin
(sgc_propagate_f32_cpu) on the same inputs, and the knob forced to v against
the knob at 0.  No tolerance anywhere."""
import functools
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 20001
K = 2
HEAVY, HUB = 64, 256   # forced thresholds: light <= 64 < pairs <= 256 < hub
HUB_NNZ = 10000        # every column group's run stays above the serial-hub limit: never fused
TS = [4, 16, 32]
WIDTHS = [602, 516, 260, 132, 130, 128]
SENTINEL = 12345.0
EMPTY_BLOCK = (100, 132)    # rows without nonzeros, in place
SHORT_BLOCK = (200, 260)    # rows of 1..3 nonzeros, in place


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgc_amd import _lib
    _lib.load()  # fails loudly if libsgc_amd.so is missing


def _set(key, value):
    from sgc_amd import _lib
    _lib.check(_lib.load().sgc_set_tuning(key.encode(), int(value)), f"set_tuning {key}")


def _get(key):
    from sgc_amd import _lib
    return int(_lib.load().sgc_get_tuning(key.encode()))


@pytest.fixture()
def knobs():
    """rows_per_wave = 2 (the multi-row kernel below its row-count rule); the
    library's and the module's schedule knobs restored afterwards."""
    mod = importlib.import_module("sgc_amd.propagate")
    saved = mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS, mod.PAD_X0
    _set("rows_per_wave", 2)
    yield mod
    mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS, mod.PAD_X0 = saved
    _set("rows_per_wave", 0)
    _set("short_wide", -1)
    _set("short_wide_first", 0)


def _csr_arrays(deg, n_cols, seed):
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(deg) + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n_cols, size=int(d), replace=False)) for d in deg]
                        + [np.zeros(0, np.int64)])
    va = rng.standard_normal(int(rp[-1])).astype(np.float32)
    return rp.astype(np.int32), ci.astype(np.int32), va


@functools.lru_cache(maxsize=None)
def _degrees():
    """20,001 rows: every length 0..40 many times (so Ts - 1, Ts, Ts + 1 for Ts
    = 4 / 16 / 32, and 17 and 33), a block of empty rows and a block of rows of
    1..3 nonzeros in place, four rows above the heavy threshold, one hub row.
    The rows of at most 4, 16 and 32 nonzeros are each an odd number, so the
    last wide wave holds a single row at every forced Ts."""
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 41, size=N)
    deg[EMPTY_BLOCK[0]:EMPTY_BLOCK[1]] = 0
    deg[SHORT_BLOCK[0]:SHORT_BLOCK[1]] = rng.integers(1, 4, size=SHORT_BLOCK[1] - SHORT_BLOCK[0])
    special = 1000 + 37 * np.arange(5)
    deg[special[:4]] = [70, 97, 128, 200]
    deg[special[4]] = HUB_NNZ
    deg[0], deg[N - 1] = 40, 0  # a long light row first, an empty row last
    free = 5000  # rows from here on are adjusted for the parities
    for lo, hi, fix in [(0, 4, 2), (5, 16, 9), (17, 32, 20)]:
        if int(((deg >= lo) & (deg <= hi)).sum()) % 2 == (0 if lo == 0 else 1):
            j = free + int(np.argmax(deg[free:] > 32))
            deg[j] = fix  # one more row in this class (taken from the rows above 32)
    for ts in TS:
        assert int((deg <= ts).sum()) % 2 == 1, ts
    for d in [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33]:
        assert (deg == d).any(), d
    return deg


@functools.lru_cache(maxsize=None)
def _graph():
    return _csr_arrays(_degrees(), N, 11)


@pytest.fixture(scope="module")
def csr():
    from sgc_amd.propagate import DeviceCSR
    c = DeviceCSR.from_host_arrays(*_graph(), device=DEV)
    assert c.cols_ascending
    return c


def _twin(arrays, X, hops=K):
    from sgc_amd.propagate import DeviceCSR, propagate
    want = propagate(DeviceCSR.from_host_arrays(*arrays, device="cpu"), torch.from_numpy(X), hops)
    return want.numpy()


@functools.lru_cache(maxsize=None)
def _case(F):
    """(X, S^K X by the CPU twin) at width F; computed once, never modified."""
    X = np.random.default_rng(F).standard_normal((N, F)).astype(np.float32)
    want = _twin(_graph(), X)
    X.setflags(write=False)
    want.setflags(write=False)
    return X, want


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got.cpu().numpy() if isinstance(got, torch.Tensor) else got),
                          _bits(want))


def _propagate(csr, X, out=None, **kw):
    from sgc_amd.propagate import propagate
    got = propagate(csr, X, K, out=out, threshold=HEAVY, hub_threshold=HUB, **kw)
    torch.cuda.synchronize()
    return got


def _padded(F, fill=0.0):
    ld = (F + 31) // 32 * 32
    return torch.full((N, ld), fill, dtype=torch.float32, device=DEV)


def _layout_run(mod, csr, X, F, layout):
    """K = 2 through one of three layouts; returns X_K [N, F] on the device."""
    from sgc_amd.propagate import SPMM_X_PADDED, SPMM_Y_PADDED, spmm
    Xh = torch.tensor(X)
    if layout == "padded":  # hop by hop, both ends the engine's 128-B-row buffers
        a, b = _padded(F), _padded(F)
        a[:, :F] = Xh.to(DEV)
        for _ in range(K):
            spmm(csr, a[:, :F], out=b[:, :F], threshold=HEAVY, hub_threshold=HUB,
                 flags=SPMM_X_PADDED | SPMM_Y_PADDED)
            a, b = b, a
        torch.cuda.synchronize()
        return a[:, :F].clone()
    if layout == "caller":  # re-laid X_0, the last hop into a caller's contiguous [N, F]
        mod.PAD_X0 = True
        out = torch.full((N, F), SENTINEL, dtype=torch.float32, device=DEV)
        return _propagate(csr, Xh.to(DEV), out)
    assert layout == "x8"  # a caller's 8-B-aligned X_0 straight into hop 1
    mod.PAD_X0 = None
    flat = torch.zeros(N * F + 8, dtype=torch.float32, device=DEV)
    Xd = flat[2:2 + N * F].view(N, F)
    Xd.copy_(Xh)
    assert Xd.data_ptr() % 16 == 8
    return _propagate(csr, Xd)


def test_plan_has_every_path(csr):
    pl = csr.plan(0, N, HEAVY, HUB, 602)
    assert pl.n_hub == 1 and pl.n_heavy == 5 and pl.max_hub_degree == HUB_NNZ
    assert pl.hub_flags() & 32 == 0, "the hub row must not be a serial (fused) one"


@pytest.mark.parametrize("rng", [(0, N), (4321, 15001), EMPTY_BLOCK, SHORT_BLOCK, (0, 0)])
def test_plan_counts_equal_host_counts(csr, rng):
    """sgc_plan_sorted_ex2's counts against row_ptr on the host: whole graph, a
    row range, a range of only empty rows, one with no row above 4 nonzeros."""
    from sgc_amd.propagate import wide_args
    rb, re = rng
    deg = _degrees()[rb:re]
    pl = csr.plan(rb, re, HEAVY, HUB, 602)
    if re > rb:
        assert pl.above == tuple(int((deg > t).sum()) for t in (4, 8, 16, 32))
        assert pl.n_nonempty == int((deg > 0).sum())
    assert pl.n_heavy == int((deg > HEAVY).sum())
    for ts in [4, 8, 16, 32, 5, 1]:  # 5 and 1: counted from row_ptr, not by the plan
        want = int(((deg > ts) & (deg <= HEAVY)).sum())
        got = wide_args(csr, pl, rb, re, ts)
        assert got == ((want, ts) if re > rb and pl.ordered else (-1, 0)), (rng, ts)
    assert wide_args(csr, pl, rb, re, 0) == (-1, 0)


@pytest.mark.parametrize("layout", ["padded", "caller", "x8"])
@pytest.mark.parametrize("ts", TS)
@pytest.mark.parametrize("F", WIDTHS)
def test_widths_and_layouts(csr, knobs, F, ts, layout):
    """K = 2 equals the twin with the knob forced and with it off, and so the
    two equal each other; the wide path runs above one slice and only there."""
    X, want = _case(F)
    _set("short_wide", ts)
    before = _get("short_wide_launches")
    got = _layout_run(knobs, csr, X, F, layout)
    took = _get("short_wide_launches") - before
    _set("short_wide", 0)
    off = _layout_run(knobs, csr, X, F, layout)
    assert _get("short_wide_launches") == before + took, "short_wide = 0 took wide items"
    assert torch.equal(got, off), (F, ts, layout)
    assert _same(got, want), (F, ts, layout)
    if F == 128:
        assert took == 0, "one slice: the wide path must not engage"
    elif layout == "padded":
        assert took == K, (F, ts, took)
    else:
        assert took >= 1, (F, ts, layout)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("ts", [4, 7, 16, 32])
def test_all_light_rows_wide_no_heavy(knobs, ts, first):
    """3,001 rows of 0..4 nonzeros: no per-slice workgroup exists at all."""
    from sgc_amd.propagate import DeviceCSR
    n, F = 3001, 602
    arrays = _csr_arrays(np.random.default_rng(3).integers(0, 5, size=n), n, 5)
    X = np.random.default_rng(1).standard_normal((n, F)).astype(np.float32)
    c = DeviceCSR.from_host_arrays(*arrays, device=DEV)
    knobs.PAD_X0 = True
    _set("short_wide", ts)
    _set("short_wide_first", first)
    before = _get("short_wide_launches")
    got = _propagate(c, torch.tensor(X).to(DEV))
    assert _get("short_wide_launches") == before + K
    assert _same(got, _twin(arrays, X)), (ts, first)


def test_wide_workgroups_first(csr, knobs):
    X, want = _case(602)
    knobs.PAD_X0 = True
    _set("short_wide", 16)
    _set("short_wide_first", 1)
    assert _same(_propagate(csr, torch.tensor(X).to(DEV)), want)


def test_no_wide_row_at_all(knobs):
    """Every row has 17..40 nonzeros: at Ts = 16 the count equals the light
    count and the launch is the ordinary one."""
    from sgc_amd.propagate import DeviceCSR, wide_args
    n, F = 2049, 260
    arrays = _csr_arrays(np.random.default_rng(4).integers(17, 41, size=n), n, 6)
    X = np.random.default_rng(2).standard_normal((n, F)).astype(np.float32)
    c = DeviceCSR.from_host_arrays(*arrays, device=DEV)
    pl = c.plan(0, n, HEAVY, HUB, F)
    assert wide_args(c, pl, 0, n, 16) == (n - pl.n_heavy, 16)
    knobs.PAD_X0 = True
    _set("short_wide", 16)
    before = _get("short_wide_launches")
    got = _propagate(c, torch.tensor(X).to(DEV))
    assert _get("short_wide_launches") == before
    assert _same(got, _twin(arrays, X))


@pytest.mark.parametrize("ts", TS)
def test_empty_row_beside_a_row_of_exactly_ts(knobs, ts):
    """The wide stretch is [one row of Ts nonzeros, three empty rows]: the
    first wide wave pairs the Ts row with an empty one, the second holds only
    empty rows (written as zeros)."""
    from sgc_amd.propagate import DeviceCSR
    n, F = 515, 602
    deg = np.random.default_rng(ts).integers(ts + 1, 50, size=n)
    deg[[7, 100, 300, 514]] = [0, ts, 0, 0]
    arrays = _csr_arrays(deg, n, 8)
    X = np.random.default_rng(3).standard_normal((n, F)).astype(np.float32)
    c = DeviceCSR.from_host_arrays(*arrays, device=DEV)
    knobs.PAD_X0 = True
    _set("short_wide", ts)
    before = _get("short_wide_launches")
    out = torch.full((n, F), SENTINEL, dtype=torch.float32, device=DEV)
    got = _propagate(c, torch.tensor(X).to(DEV), out)
    assert _get("short_wide_launches") == before + K
    assert _same(got, _twin(arrays, X)), ts


@pytest.mark.parametrize("ts", [4, 16])
def test_row_range(csr, knobs, ts):
    """One hop over rows [4321, 15001) in the padded layout."""
    from sgc_amd.propagate import SPMM_X_PADDED, SPMM_Y_PADDED, DeviceCSR, spmm
    F, rb, re = 516, 4321, 15001
    X, _ = _case(F)
    want = spmm(DeviceCSR.from_host_arrays(*_graph(), device="cpu"), torch.tensor(X), rb, re)
    a = _padded(F)
    a[:, :F] = torch.tensor(X).to(DEV)
    y = torch.full((re - rb, a.shape[1]), SENTINEL, dtype=torch.float32, device=DEV)
    _set("short_wide", ts)
    before = _get("short_wide_launches")
    spmm(csr, a[:, :F], rb, re, out=y[:, :F], threshold=HEAVY, hub_threshold=HUB,
         flags=SPMM_X_PADDED | SPMM_Y_PADDED)
    torch.cuda.synchronize()
    assert _get("short_wide_launches") == before + 1
    assert torch.equal(y[:, :F].cpu(), want), ts


@pytest.mark.parametrize("whole", [0, None])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("ts", [4, 16, 32])
@pytest.mark.parametrize("F", [602, 130])
def test_accumulate_launches(csr, knobs, F, ts, G, whole):
    """Column groups: with the pure split (whole = 0) short runs, and rows
    whose run in a group is empty, reach the accumulate launches as wide
    items; None is the default whole-row rule (T = 32)."""
    knobs.COLUMN_GROUPS, knobs.GROUP_WHOLE_ROWS, knobs.PAD_X0 = G, whole, True
    X, want = _case(F)
    _set("short_wide", ts)
    before = _get("short_wide_launches")
    got = _propagate(csr, torch.tensor(X).to(DEV))
    took = _get("short_wide_launches") - before
    assert _same(got, want), (F, ts, G, whole)
    assert took >= K * (G if whole == 0 else 1), (took, F, ts, G, whole)
    _set("short_wide", 0)
    assert torch.equal(_propagate(csr, torch.tensor(X).to(DEV)), got)


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("ts", [4, 16])
def test_goldens_with_the_knob_forced(tiny_cases, knobs, G, ts):
    from sgc_amd.propagate import DeviceCSR, propagate
    knobs.COLUMN_GROUPS = G
    _set("short_wide", ts)
    for name, c in tiny_cases.items():
        n = int(c["n"])
        idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64))
        adj = torch.sparse_coo_tensor(idx, torch.from_numpy(c["vals"]), (n, n)).to(DEV)
        dcsr = DeviceCSR.from_torch(adj)
        X = torch.from_numpy(c["X"]).to(DEV)
        for key in sorted(k for k in c if k.startswith("Y") and int(k[1:]) > 0):
            got = propagate(dcsr, X, int(key[1:]))
            assert _same(got, c[key]), (name, key, G, ts)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("F", [602, 130])
def test_guards_flat_output_and_poisoned_gaps(csr, knobs, F, G):
    """`out` is an [N, F] view one float into a flat sentinel buffer (4-byte
    aligned rows); X is the [:, :F] view of an [N, F + 3] buffer whose gap
    columns hold NaN.  Nothing at or beyond column F is read into a result or
    written."""
    knobs.COLUMN_GROUPS, knobs.PAD_X0 = G, True
    X, want = _case(F)
    xbuf = torch.full((N, F + 3), float("nan"), dtype=torch.float32, device=DEV)
    xbuf[:, :F] = torch.tensor(X).to(DEV)
    oflat = torch.full((N * F + 9,), SENTINEL, dtype=torch.float32, device=DEV)
    out = oflat[1:1 + N * F].view(N, F)
    assert out.data_ptr() % 8 == 4
    _set("short_wide", 16)
    before = _get("short_wide_launches")
    _propagate(csr, xbuf[:, :F], out)
    assert _get("short_wide_launches") >= before + K
    got = oflat.cpu().numpy()
    assert np.array_equal(_bits(got[1:1 + N * F]).reshape(N, F), _bits(want)), (F, G)
    guard = np.concatenate([got[:1], got[1 + N * F:]])
    assert np.array_equal(_bits(guard), _bits(np.full(9, SENTINEL, np.float32))), (F, G)
    gap = torch.full((N, F + 3), SENTINEL, dtype=torch.float32, device=DEV)
    _propagate(csr, xbuf[:, :F], gap[:, :F])
    g = gap.cpu().numpy()
    assert np.array_equal(_bits(g[:, :F]), _bits(want)), (F, G)
    assert np.array_equal(_bits(g[:, F:]), _bits(np.full((N, 3), SENTINEL, np.float32))), (F, G)


def test_recorded_list_graph_and_native_loop_equal_direct(knobs):
    """A small graph (its intermediates fit a recorded launch list): the second
    call of propagate() replays the list, GraphedPropagation a captured graph,
    native_loop the C loop; all equal the direct call and take wide items."""
    from sgc_amd.propagate import DeviceCSR, GraphedPropagation, propagate
    n, F = 4099, 260
    deg = np.random.default_rng(9).integers(0, 41, size=n)
    deg[5] = 3500  # above the serial-hub limit: the hub kernel is not fused
    arrays = _csr_arrays(deg, n, 10)
    X = np.random.default_rng(4).standard_normal((n, F)).astype(np.float32)
    want = _twin(arrays, X)
    c = DeviceCSR.from_host_arrays(*arrays, device=DEV)
    Xd = torch.tensor(X).to(DEV)
    knobs.PAD_X0 = True
    _set("short_wide", 16)
    kw = dict(threshold=HEAVY, hub_threshold=HUB)
    counts = [_get("short_wide_launches")]
    direct = propagate(c, Xd, K, prepare=False, **kw)
    counts.append(_get("short_wide_launches"))
    first = propagate(c, Xd, K, **kw)    # records
    counts.append(_get("short_wide_launches"))
    second = propagate(c, Xd, K, **kw)   # replays
    counts.append(_get("short_wide_launches"))
    assert any(isinstance(k, tuple) and k[:1] == ("list",) for k in c._plans), "no list recorded"
    native = propagate(c, Xd, K, native_loop=True, **kw)
    counts.append(_get("short_wide_launches"))
    torch.cuda.synchronize()
    assert [b - a for a, b in zip(counts, counts[1:])] == [K, K, K, K]
    for got in (direct, first, second, native):
        assert _same(got, want)
    gp = GraphedPropagation(c, (n, F), K, **kw)
    got = gp.run(Xd)
    torch.cuda.synchronize()
    assert _same(got, want)

    # toggling the knob does not replay a list recorded under the other value
    _set("short_wide", 0)
    before = _get("short_wide_launches")
    off = propagate(c, Xd, K, **kw)
    torch.cuda.synchronize()
    assert _get("short_wide_launches") == before, "a list recorded with wide items was replayed"
    assert _same(off, want)
    _set("short_wide", 16)
    on = propagate(c, Xd, K, **kw)
    torch.cuda.synchronize()
    assert _get("short_wide_launches") == before + K
    assert _same(on, want)


def test_knob_values():
    from sgc_amd import _lib
    lib = _lib.load()
    assert _get("short_wide") == -1 and _get("short_wide_ts") == 16
    assert lib.sgc_set_tuning(b"short_wide", 33) != 0 and lib.sgc_set_tuning(b"short_wide", -2) != 0
    _set("short_wide", 0)
    assert _get("short_wide_ts") == 0
    _set("short_wide", 7)
    assert _get("short_wide") == 7 and _get("short_wide_ts") == 7
    _set("short_wide", -1)
