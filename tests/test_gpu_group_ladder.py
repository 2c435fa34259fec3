"""Column groups by row length (sgc_csr_colsplit_ex2, the "length ladder"): a
row of more than H nonzeros is cut at all G column cuts, a row of T+1..H only
at the Gc coarse cuts (its runs in fine groups 0, G/Gc, ...), a row of at most
T stays whole in group 0.  A schedule only, so everything here is bit-exact."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

from test_gpu_parity import bits_equal, coo_cuda

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgc_amd import _lib
    _lib.load()  # fails loudly if libsgc_amd.so is missing


KNOBS = ("COLUMN_GROUPS", "GROUP_WHOLE_ROWS", "GROUP_COARSE_ROWS", "GROUP_COARSE_GROUPS", "PAD_X0")


@pytest.fixture()
def prop_mod():
    """sgc_amd.propagate with its group knobs restored afterwards."""
    mod = importlib.import_module("sgc_amd.propagate")
    saved = [getattr(mod, k) for k in KNOBS]
    yield mod
    for k, v in zip(KNOBS, saved):
        setattr(mod, k, v)


def _force(mod, G, Gc, H, T):
    mod.COLUMN_GROUPS, mod.GROUP_COARSE_GROUPS = G, Gc
    mod.GROUP_COARSE_ROWS, mod.GROUP_WHOLE_ROWS = H, T


def _csr_from_rows(rows):
    """Host CSR arrays from a list of (cols, vals) per row."""
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(c) for c, _ in rows], out=rp[1:])
    ci = np.concatenate([np.asarray(c, np.int32) for c, _ in rows]).astype(np.int32)
    va = np.concatenate([np.asarray(v, np.float32) for _, v in rows]).astype(np.float32)
    return rp.astype(np.int32), ci, va


def _split_host_ladder(rp, ci, va, n_cols, G, T, H, Gc):
    """The ladder on the host.  Every nonzero's fine group is the column range
    [g * n_cols / G, (g + 1) * n_cols / G) it lies in; a row of at most T
    nonzeros has everything in group 0, a row of T+1..H rounds the fine group
    down to a multiple of G / Gc, a longer row keeps it.  Group-major arrays,
    absolute row_ptrs."""
    n = rp.shape[0] - 1
    step = G // Gc
    cuts = np.asarray([(g * n_cols) // G for g in range(G + 1)])
    length = np.diff(rp.astype(np.int64))
    row = np.repeat(np.arange(n), length)
    grp = np.searchsorted(cuts[1:], ci, side="right")
    medium = (length[row] > T) & (length[row] <= H)
    grp[medium] = grp[medium] // step * step
    grp[length[row] <= T] = 0
    rps, cols, vals, base = [], [], [], 0
    for g in range(G):
        keep = grp == g
        cnt = np.bincount(row[keep], minlength=n)
        rps.append(base + np.concatenate([[0], np.cumsum(cnt)]))
        cols.append(ci[keep])
        vals.append(va[keep])
        base += int(keep.sum())
    return np.stack(rps).astype(np.int32), np.concatenate(cols), np.concatenate(vals)


SPLIT_T, SPLIT_H, SPLIT_N = 2, 5, 300


@functools.lru_cache(maxsize=None)
def _split_graph():
    """300 rows over 300 columns for T = 2, H = 5: random rows of 0..12
    nonzeros, then by hand empty rows, rows of T-1 / T / T+1 and H-1 / H / H+1
    nonzeros, a hub row (every column), a heavy row with all its nonzeros in
    the last fine range of G = 4 / 6 / 8, a heavy row whose middle ranges are
    empty, and a medium row with nothing in the first coarse range."""
    n = SPLIT_N
    rng = np.random.default_rng(31)

    def row(cols):
        cols = np.sort(np.asarray(cols, np.int64))
        return cols, rng.standard_normal(len(cols))
    rows = [row(rng.choice(n, size=int(k), replace=False)) for k in rng.integers(0, 13, size=n)]
    for r in (0, 17, n - 1):
        rows[r] = row([])
    for r, k in zip(range(20, 26), (1, 2, 3, 4, 5, 6)):
        rows[r] = row(rng.choice(n, size=k, replace=False))
    rows[30] = row(np.arange(n))                                     # hub
    rows[31] = row(270 + rng.choice(30, size=8, replace=False))      # heavy, last fine range
    rows[32] = row(np.concatenate([rng.choice(37, size=4, replace=False),
                                   270 + rng.choice(30, size=4, replace=False)]))  # empty middle
    rows[33] = row(160 + rng.choice(140, size=4, replace=False))     # medium, upper half only
    rows[34] = row(rng.choice(37, size=5, replace=False))            # medium, first range only
    return _csr_from_rows(rows)


@pytest.mark.parametrize("G", [4, 6, 8])
def test_colsplit_ex2_matches_host_rule(G):
    """row_ptrs, col and val of sgc_csr_colsplit_ex2 against the numpy rule,
    exactly, at Gc = 1 / 2 / G; Gc = G is sgc_csr_colsplit_ex's split."""
    from sgc_amd.propagate import DeviceCSR
    rp, ci, va = _split_graph()
    n, T, H = SPLIT_N, SPLIT_T, SPLIT_H
    length = np.diff(rp.astype(np.int64))
    assert {0, T - 1, T, T + 1, H - 1, H, H + 1, n} <= set(length.tolist())
    csr = DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)
    assert csr.cols_ascending
    for Gc in (1, 2, G):
        subs = csr.column_groups(G, T, H, Gc)
        torch.cuda.synchronize()
        want_rp, want_ci, want_va = _split_host_ladder(rp, ci, va, n, G, T, H, Gc)
        got_rp = np.stack([s.row_ptr.cpu().numpy() for s in subs])
        assert np.array_equal(got_rp, want_rp), (G, Gc)
        assert np.array_equal(subs[0].col_idx.cpu().numpy(), want_ci), (G, Gc)
        assert bits_equal(subs[0].val.cpu().numpy(), want_va), (G, Gc)
        deg = np.diff(got_rp.astype(np.int64), axis=1)  # [G, n] run lengths
        step = G // Gc
        off = [g for g in range(G) if g % step]
        medium = (length > T) & (length <= H)
        assert not deg[1:, length <= T].any() and not deg[off][:, medium].any(), (G, Gc)
        assert not deg[:G - 1, 31].any() and deg[G - 1, 31] == 8      # last fine range only
        assert deg[0, 32] == 4 and deg[G - 1, 32] == 4                # empty middle ranges
        if Gc == 2:
            assert deg[0, 33] == 0 and deg[G // 2, 33] == 4           # no first coarse run
        if Gc == G:
            assert subs is csr.column_groups(G, T)
    assert len([k for k in csr._plans if k[:1] == ("groups",)]) == 3
    csr.drop_groups()
    assert not [k for k in csr._plans if k[:1] == ("groups",)]


def test_colsplit_ex2_argument_errors():
    """Gc not dividing G, Gc < 1, H < T and null pointers return SGC_EINVAL
    and launch nothing: the outputs keep their fill."""
    from sgc_amd import _lib
    lib = _lib.load()
    rp, ci, va = _split_graph()
    n, nnz, G = SPLIT_N, int(rp[-1]), 4
    d = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    rpd, cid, vad = d(rp), d(ci), d(va)
    cuts = (ctypes.c_int32 * (G + 1))(*[(g * n) // G for g in range(G + 1)])
    row_ptrs = torch.full((G, n + 1), -7, dtype=torch.int32, device=DEV)
    col = torch.full((nnz,), -7, dtype=torch.int32, device=DEV)
    val = torch.full((nnz,), SENTINEL, dtype=torch.float32, device=DEV)
    ws_bytes = lib.sgc_colsplit_workspace(n, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def call(T=2, H=5, Gc=2, row_ptr=rpd, out_rp=row_ptrs, cuts_p=cuts, work=ws):
        return lib.sgc_csr_colsplit_ex2(
            _lib.ptr(row_ptr), _lib.ptr(cid), _lib.ptr(vad), n, n, G,
            ctypes.cast(cuts_p, ctypes.c_void_p) if cuts_p is not None else None, T, H, Gc,
            _lib.ptr(out_rp), _lib.ptr(col), _lib.ptr(val), _lib.ptr(work), ws_bytes,
            _lib.stream_handle(torch.device(DEV)))
    EINVAL = 1
    assert call(Gc=3) == EINVAL          # 3 does not divide 4
    assert call(Gc=0) == EINVAL
    assert call(Gc=-2) == EINVAL
    assert call(Gc=8) == EINVAL          # a multiple, not a divisor
    assert call(T=6, H=5) == EINVAL      # H < T
    assert call(T=-1, H=5) == EINVAL
    assert call(row_ptr=None) == EINVAL
    assert call(out_rp=None) == EINVAL
    assert call(cuts_p=None) == EINVAL
    assert call(work=None) == EINVAL
    assert b"colsplit" in lib.sgc_last_error()
    torch.cuda.synchronize()
    assert bool((row_ptrs == -7).all()) and bool((col == -7).all())
    assert bool((val == SENTINEL).all())
    assert call() == 0 and call(T=5, H=5, Gc=1) == 0  # H == T: no medium rows
    torch.cuda.synchronize()
    assert int(row_ptrs[G - 1, n]) == nnz


@pytest.mark.parametrize("G,Gc", [(4, 2), (8, 2), (6, 3), (3, 1)])
def test_ladder_tiny_cases_bit_exact(tiny_cases, prop_mod, G, Gc):
    """Every golden case through propagate() with the ladder forced (T = 2,
    H = 5: whole, medium and heavy rows on 48-row graphs), K = 1 and 3: the
    hop loop that records the launch list, its replay, and the native loop
    all give the goldens' bits."""
    from sgc_amd.propagate import DeviceCSR, group_ladder_for, propagate
    _force(prop_mod, G, Gc, 5, 2)
    classes = set()
    for name, c in tiny_cases.items():
        csr = DeviceCSR.from_torch(coo_cuda(c))
        X = torch.from_numpy(c["X"]).to(DEV)
        n = int(c["n"])
        laddered = csr.cols_ascending and csr.nnz > 0 and n >= G  # else one group
        if laddered:
            assert group_ladder_for(csr, X.shape[1]) == (G, Gc, 5), name
        length = np.diff(csr.row_ptr.cpu().numpy().astype(np.int64))
        classes |= set(np.digitize(length, [2.5, 5.5]).tolist())
        for K in (1, 3):
            if f"Y{K}" not in c:
                continue
            want = c[f"Y{K}"]
            first = propagate(csr, X, K)
            again = propagate(csr, X, K)
            native = propagate(csr, X, K, native_loop=True)
            torch.cuda.synchronize()
            if laddered:
                assert any(isinstance(k, tuple) and k[:1] == ("list",) for k in csr._plans), name
                assert any(k[:1] == ("groups",) and len(k) == 5 for k in csr._plans
                           if isinstance(k, tuple)), name
            assert bits_equal(first.cpu().numpy(), want), (name, K, "loop")
            assert bits_equal(again.cpu().numpy(), want), (name, K, "launch list")
            assert bits_equal(native.cpu().numpy(), want), (name, K, "native")
    assert classes == {0, 1, 2}


MEDIUM_N, MEDIUM_EDGES = 70000, 1_000_000


@functools.lru_cache(maxsize=None)
def _medium_graph():
    """One seeded R-MAT graph: 70,000 rows, ~2.07 M nonzeros."""
    from sgc_amd import graphs
    S = graphs.synthetic_graph("reddit", seed=5, n=MEDIUM_N, edges=MEDIUM_EDGES)
    return S.row_ptr, S.col_idx, S.val


@functools.lru_cache(maxsize=None)
def _medium_case(F):
    """(X, S X, S^2 X) by the CPU twin at width F; computed once, read-only."""
    from sgc_amd.propagate import DeviceCSR, propagate
    rp, ci, va = _medium_graph()
    host = DeviceCSR.from_host_arrays(rp, ci, va, device="cpu")
    X = np.random.default_rng(F).standard_normal((MEDIUM_N, F)).astype(np.float32)
    Y1 = propagate(host, torch.from_numpy(X), 1).numpy()
    Y2 = propagate(host, torch.from_numpy(Y1), 1).numpy()
    for a in (X, Y1, Y2):
        a.setflags(write=False)
    return X, Y1, Y2


@functools.lru_cache(maxsize=None)
def _medium_split(G):
    """The host rule's row_ptrs of the medium graph at (G, 2, 64), T = 32."""
    rp, ci, va = _medium_graph()
    return _split_host_ladder(rp, ci, va, MEDIUM_N, G, 32, 64, 2)[0]


@pytest.fixture(scope="module")
def medium_csr():
    from sgc_amd.propagate import DeviceCSR
    rp, ci, va = _medium_graph()
    assert 1_900_000 < rp[-1] < (1 << 22)  # the size rule alone would keep G = 1
    return DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)


@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("F", [602, 130, 128])
def test_ladder_medium_graph_bit_exact(medium_csr, prop_mod, F, G):
    """The multi-row kernel with wide items (70 K rows) at 602 / 130 / 128
    floats under (G, Gc, H) = (4, 2, 64) and (8, 2, 64), T = 32: K = 1 and
    K = 2 through propagate() equal the CPU twin, and so does the same call
    replayed from its launch list with other contents in X."""
    from sgc_amd.propagate import propagate
    csr = medium_csr
    _force(prop_mod, G, 2, 64, 32)
    X, Y1, Y2 = _medium_case(F)
    Xd = torch.from_numpy(X).to(DEV)
    lists = lambda: [k for k in csr._plans if isinstance(k, tuple) and k[:1] == ("list",)]  # noqa: E731
    csr.release_prepared()
    out1 = torch.full((MEDIUM_N, F), SENTINEL, dtype=torch.float32, device=DEV)
    propagate(csr, Xd, 1, out=out1)  # records
    torch.cuda.synchronize()
    assert len(lists()) == 1
    parts = csr._plans[("groups", G, 32, 64, 2)]
    plans = [p.plan(0, MEDIUM_N, None, None, F) for p in parts]
    want_rp = _medium_split(G)
    length = np.diff(_medium_graph()[0].astype(np.int64))
    for g, (part, pl) in enumerate(zip(parts, plans)):
        assert np.array_equal(part.row_ptr.cpu().numpy(), want_rp[g]), (G, g)
        deg = np.diff(want_rp[g].astype(np.int64))
        assert pl.ordered and pl.n_nonempty == int((deg > 0).sum()) > 0, (G, g)
        if g % (G // 2):  # a fine-only group: runs of the rows above 64 and nothing else
            assert not deg[length <= 64].any() and deg[length > 64].any(), (G, g)
    assert bits_equal(out1.cpu().numpy(), Y1), (F, G, "K=1 loop")
    Xd.copy_(torch.from_numpy(Y1))  # other contents, same tensors: the replay
    propagate(csr, Xd, 1, out=out1)
    torch.cuda.synchronize()
    assert len(lists()) == 1
    assert bits_equal(out1.cpu().numpy(), Y2), (F, G, "K=1 launch list")
    Xd.copy_(torch.from_numpy(X))
    out2 = propagate(csr, Xd, 2)
    again = propagate(csr, Xd, 2)
    torch.cuda.synchronize()
    assert bits_equal(out2.cpu().numpy(), Y2), (F, G, "K=2")
    assert bits_equal(again.cpu().numpy(), Y2), (F, G, "K=2 again")
    csr.drop_groups()


RAGGED_N, RAGGED_F = 4096, 602
HEAVY, HUB = 64, 256  # forced thresholds: light <= 64 < pairs <= 256 < hub


@functools.lru_cache(maxsize=None)
def _ragged_graph():
    """4,096 rows: mostly short, 120 rows of 33..64 nonzeros (medium at H =
    64), twelve of 400..800 and one of 1,500 (heavy: their runs in every one of
    four fine groups stay above the heavy threshold), forty empty rows."""
    n = RAGGED_N
    rng = np.random.default_rng(77)
    deg = rng.integers(1, 24, size=n)
    deg[rng.choice(n, size=120, replace=False)] = rng.integers(33, 65, size=120)
    special = rng.choice(n, size=53, replace=False)
    deg[special[:12]] = rng.integers(400, 801, size=12)
    deg[special[12]] = 1500
    deg[special[13:]] = 0
    deg[0], deg[n - 1] = 40, 0
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, size=d, replace=False)) for d in deg])
    va = rng.standard_normal(int(rp[-1])).astype(np.float32)
    return rp.astype(np.int32), ci.astype(np.int32), va


@pytest.mark.parametrize("K", [1, 2])
def test_heavy_only_accumulate_launch_unaligned_rows(prop_mod, K):
    """(G, Gc, H, T) = (4, 2, 64, 32): fine groups 1 and 3 hold heavy and hub
    items only, so their accumulate launches have an empty light list.  The
    last hop writes a caller's [N, 602] view one float into a flat buffer
    (4-byte aligned rows); the floats before row 0 and after row N - 1 keep
    their sentinel, X is not written, and the result is the CPU twin's."""
    from sgc_amd.propagate import DeviceCSR, propagate
    n, F = RAGGED_N, RAGGED_F
    rp, ci, va = _ragged_graph()
    _force(prop_mod, 4, 2, 64, 32)
    X = np.random.default_rng(K).standard_normal((n, F)).astype(np.float32)
    want = propagate(DeviceCSR.from_host_arrays(rp, ci, va, device="cpu"),
                     torch.from_numpy(X), K).numpy()
    csr = DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)
    parts = csr.groups_or_self(4)
    assert len(parts) == 4
    for g, part in enumerate(parts):
        pl = part.plan(0, n, HEAVY, HUB, F)
        assert pl.n_hub == 1 and pl.n_heavy == 13, (g, pl.n_heavy)
        assert (pl.accumulate_light_items == 0) == (g % 2 == 1), (g, pl.accumulate_light_items)
    xflat = torch.full((n * F + 9,), float("nan"), dtype=torch.float32, device=DEV)
    Xd = xflat[1:1 + n * F].view(n, F)
    Xd.copy_(torch.from_numpy(X))
    oflat = torch.full((n * F + 9,), SENTINEL, dtype=torch.float32, device=DEV)
    out = oflat[1:1 + n * F].view(n, F)
    assert Xd.data_ptr() % 8 == 4 and out.data_ptr() % 8 == 4
    for what in ("loop", "launch list"):
        out.fill_(SENTINEL)
        propagate(csr, Xd, K, out=out, threshold=HEAVY, hub_threshold=HUB)
        torch.cuda.synchronize()
        got = oflat.cpu().numpy()
        assert bits_equal(got[1:1 + n * F].reshape(n, F), want), (K, what)
        guard = np.concatenate([got[:1], got[1 + n * F:]])
        assert bits_equal(guard, np.full(9, SENTINEL, np.float32)), (K, what)
    assert bits_equal(Xd.cpu().numpy(), X), "X was written"


def test_rule_leaves_small_shapes_alone(prop_mod):
    """Cora and Pubmed shape come out of the rule with one group, whatever
    the ladder's own knobs say, and a forced G has no ladder unless asked."""
    from sgc_amd import graphs
    from sgc_amd.propagate import DeviceCSR, column_groups_for, group_coarse_for, group_ladder_for
    for shape in ("cora", "pubmed"):
        S = graphs.synthetic_graph(shape, seed=0)
        csr = DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device=DEV)
        F = graphs.SHAPES[shape]["features"]
        for Gc, H in ((None, None), (2, 64)):
            prop_mod.GROUP_COARSE_GROUPS, prop_mod.GROUP_COARSE_ROWS = Gc, H
            assert group_ladder_for(csr, F) == (1, 1, 0), shape
            assert column_groups_for(csr, F) == 1 and csr.groups_or_self(1)[0] is csr
    prop_mod.GROUP_COARSE_GROUPS, prop_mod.GROUP_COARSE_ROWS = None, None

    def sized(n, nnz):  # the rule reads sizes only: no graph is built
        return DeviceCSR(n, n, torch.zeros(n + 1, dtype=torch.int32, device=DEV),
                         torch.empty(nnz, dtype=torch.int32, device=DEV),
                         torch.empty(0, device=DEV), prop_mod.STATUS_COLS_ASCENDING)
    reddit = sized(232965, 23446803)
    assert group_ladder_for(reddit, 602) == (4, 2, 64)
    assert group_ladder_for(reddit, 304) == (2, 2, 32) and group_ladder_for(reddit, 128) == (2, 2, 32)
    assert group_ladder_for(reddit, 256) == (1, 1, 0)
    assert group_ladder_for(sized(60000, 4_200_000), 602) == (2, 2, 32)
    del reddit
    rmat = sized(4194304, 260194304)
    assert group_ladder_for(rmat, 256) == (8, 4, 512)
    assert group_ladder_for(rmat, 512) == (4, 4, 32) and group_ladder_for(rmat, 128) == (4, 4, 32)
    del rmat
    prop_mod.COLUMN_GROUPS, prop_mod.GROUP_WHOLE_ROWS = 4, 8
    assert group_ladder_for(csr, F) == (4, 4, 8) and group_coarse_for(csr, 4) == (4, 8)
    prop_mod.GROUP_COARSE_GROUPS = 3  # does not divide 4: ignored
    assert group_ladder_for(csr, F) == (4, 4, 8)
    prop_mod.GROUP_COARSE_GROUPS, prop_mod.GROUP_COARSE_ROWS = 2, 4  # H below T: raised to T
    assert group_ladder_for(csr, F) == (4, 2, 8)
