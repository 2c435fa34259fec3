"""Column groups with whole short rows (sgc_csr_colsplit_ex) and accumulate
launches that start no wave for a row with an empty run (sgc_plan_sorted_ex,
sgc_spmm_csr_f32_ex2): a schedule only, so everything here is bit-exact."""
import importlib

import numpy as np
import pytest
import torch

from test_gpu_parity import bits_equal, coo_cuda

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgc_amd import _lib
    _lib.load()  # fails loudly if libsgc_amd.so is missing


@pytest.fixture()
def prop_mod():
    """sgc_amd.propagate with its two group knobs restored afterwards."""
    mod = importlib.import_module("sgc_amd.propagate")
    saved = mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS
    yield mod
    mod.COLUMN_GROUPS, mod.GROUP_WHOLE_ROWS = saved


def _csr_from_rows(rows):
    """Host CSR arrays from a list of (cols, vals) per row."""
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(c) for c, _ in rows], out=rp[1:])
    ci = np.concatenate([np.asarray(c, np.int32) for c, _ in rows]).astype(np.int32)
    va = np.concatenate([np.asarray(v, np.float32) for _, v in rows]).astype(np.float32)
    return rp.astype(np.int32), ci, va


def _rows_of(S):
    return [(S.col_idx[S.row_ptr[r]:S.row_ptr[r + 1]].copy(),
             S.val[S.row_ptr[r]:S.row_ptr[r + 1]].copy()) for r in range(S.n)]


def _split_host_whole(rp, ci, va, n_cols, G, T):
    """The whole-row rule on the host: a row of at most T nonzeros is group
    0's entirely; longer rows are cut at g * n_cols / G.  Group-major arrays,
    absolute row_ptrs."""
    n = rp.shape[0] - 1
    cuts = np.asarray([(g * n_cols) // G for g in range(G + 1)])
    length = np.diff(rp.astype(np.int64))
    row = np.repeat(np.arange(n), length)
    grp = np.searchsorted(cuts[1:], ci, side="right")
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


@pytest.fixture(scope="module")
def spliced_graph():
    """A 3,000-row graph with a 3,000-nonzero row, empty rows, rows of exactly
    T-1 / T / T+1 nonzeros for T = 1, 8, 32 and a short row whose columns all
    lie in the last group's range."""
    from sgc_amd import graphs
    S = graphs.synthetic_graph("cora", seed=3, n=3000, edges=20000)
    rng = np.random.default_rng(7)
    rows = _rows_of(S)
    rows[5] = (np.arange(3000), rng.standard_normal(3000))
    for r in (10, 11, 2999):
        rows[r] = (np.empty(0, np.int32), np.empty(0, np.float32))
    for r, k in zip(range(20, 29), (0, 1, 2, 7, 8, 9, 31, 32, 33)):
        rows[r] = (np.sort(rng.choice(3000, size=k, replace=False)), rng.standard_normal(k))
    rows[40] = (np.asarray([2990, 2995, 2999]), rng.standard_normal(3))
    return _csr_from_rows(rows)


@pytest.mark.parametrize("G", [2, 3, 5])
def test_colsplit_whole_rows_matches_host_split(spliced_graph, G):
    """sgc_csr_colsplit_ex against the host rule: every group's row_ptr and
    the col / val arrays, bit for bit; T = 0 is column_groups(G), T = 10^6
    puts everything in group 0."""
    from sgc_amd.propagate import DeviceCSR
    rp, ci, va = spliced_graph
    n = rp.shape[0] - 1
    csr = DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)
    assert csr.cols_ascending
    pure = csr.column_groups(G)
    for T in (0, 1, 8, 32, 10**6):
        subs = csr.column_groups(G, T)
        torch.cuda.synchronize()
        want_rp, want_ci, want_va = _split_host_whole(rp, ci, va, n, G, T)
        for g in range(G):
            assert np.array_equal(subs[g].row_ptr.cpu().numpy(), want_rp[g]), (G, T, g)
        assert np.array_equal(subs[0].col_idx.cpu().numpy(), want_ci), (G, T)
        assert bits_equal(subs[0].val.cpu().numpy(), want_va), (G, T)
        if T == 0:
            assert subs is pure  # the two-argument call is the pure split
        if T == 10**6:
            assert np.array_equal(subs[0].row_ptr.cpu().numpy(), rp)
            assert np.array_equal(subs[0].col_idx.cpu().numpy(), ci)
            for g in range(1, G):
                assert np.all(subs[g].row_ptr.cpu().numpy() == rp[-1])
    assert len([k for k in csr._plans if k[:1] == ("groups",)]) == 5
    csr.drop_groups()
    assert not [k for k in csr._plans if k[:1] == ("groups",)]


@pytest.mark.parametrize("G", [2, 3, 4])
def test_whole_rows_tiny_cases_bit_exact(tiny_cases, prop_mod, G):
    """propagate() and sgc_precompute() with G groups and T forced: every
    golden case at every golden K matches the goldens' bits; one case also
    through the native loop."""
    from sgc_amd.propagate import DeviceCSR, propagate
    from sgc_amd.utils import sgc_precompute
    prop_mod.COLUMN_GROUPS = G
    for T in (1, 8, 32):
        prop_mod.GROUP_WHOLE_ROWS = T
        for name, c in tiny_cases.items():
            adj = coo_cuda(c)
            csr = DeviceCSR.from_torch(adj)
            X = torch.from_numpy(c["X"]).to(DEV)
            for key in sorted(k for k in c if k.startswith("Y") and k != "Y0"):
                K = int(key[1:])
                out = propagate(csr, X, K)
                pre, _ = sgc_precompute(X, adj, K)
                torch.cuda.synchronize()
                assert bits_equal(out.cpu().numpy(), c[key]), (name, key, G, T)
                assert bits_equal(pre.cpu().numpy(), c[key]), (name, key, G, T, "precompute")
        c = tiny_cases["norm_n48_F602"]
        csr = DeviceCSR.from_torch(coo_cuda(c))
        native = propagate(csr, torch.from_numpy(c["X"]).to(DEV), 2, native_loop=True)
        torch.cuda.synchronize()
        assert bits_equal(native.cpu().numpy(), c["Y2"]), (G, T, "native")


@pytest.fixture(scope="module")
def medium_graph():
    """60,000 rows, ~4.2 M nonzeros (hub, heavy and short rows), 40 rows
    emptied."""
    from sgc_amd import graphs
    n = 60000
    S = graphs.synthetic_graph("pubmed", seed=11, n=n, edges=2_100_000)
    length = np.diff(S.row_ptr.astype(np.int64))
    empty = np.random.default_rng(5).choice(n, size=40, replace=False)
    keep = np.ones(S.nnz, bool)
    for r in empty:
        keep[S.row_ptr[r]:S.row_ptr[r + 1]] = False
    length[empty] = 0
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(length, out=rp[1:])
    return n, rp.astype(np.int32), S.col_idx[keep], S.val[keep], np.sort(empty)


@pytest.mark.parametrize("F", [602, 130, 128])
def test_whole_rows_medium_graph_bit_exact(oracle, medium_graph, prop_mod, F):
    """Hub, heavy and short rows in one launch at 602 (unaligned last hop,
    scalar Y), 130 (8-byte lanes) and 128 floats (a single slice), G = 2 / 3,
    T = 8 / 32: K = 2, a row-range hop and a K = 1 call into a sentinel-filled
    `out` (rows without nonzeros come out as exact zeros): the oracle's bits."""
    from sgc_amd.propagate import DeviceCSR, propagate, spmm
    n, rp, ci, va, empty = medium_graph
    assert rp[-1] >= prop_mod.GROUPS_MIN_NNZ
    X = np.random.default_rng(F).standard_normal((n, F)).astype(np.float32)
    want1 = oracle.spmm_csr(rp, ci, va, X, 0, n)
    want2 = oracle.spmm_csr(rp, ci, va, want1, 0, n)
    assert not want1[empty].any()
    csr = DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)
    Xd = torch.from_numpy(X).to(DEV)
    for G in (2, 3):
        for T in (8, 32):
            prop_mod.COLUMN_GROUPS, prop_mod.GROUP_WHOLE_ROWS = G, T
            out2 = propagate(csr, Xd, 2)
            part = spmm(csr, Xd, 1000, 37000)
            out1 = torch.full((n, F), 12345.0, dtype=torch.float32, device=DEV)
            propagate(csr, Xd, 1, out=out1)
            torch.cuda.synchronize()
            assert ("groups", G, T) in csr._plans
            assert bits_equal(out2.cpu().numpy(), want2), (F, G, T)
            assert bits_equal(part.cpu().numpy(), want1[1000:37000]), (F, G, T, "range")
            got1 = out1.cpu().numpy()
            assert bits_equal(got1, want1), (F, G, T, "K=1")
            assert not got1[empty].view(np.uint32).any(), (F, G, T, "empty rows")
        csr.drop_groups()


def test_whole_rows_launch_list_replay(prop_mod):
    """A Pubmed-size graph with G and T forced: the second call, with new X
    contents, runs through the recorded launch list and equals the hop loop."""
    from sgc_amd import graphs
    from sgc_amd.propagate import DeviceCSR, propagate
    S = graphs.synthetic_graph("pubmed", seed=2)
    F = graphs.SHAPES["pubmed"]["features"]
    prop_mod.COLUMN_GROUPS, prop_mod.GROUP_WHOLE_ROWS = 2, 8
    csr = DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device=DEV)
    X = torch.randn((S.n, F), generator=torch.Generator().manual_seed(1)).to(DEV)
    lists = lambda: [k for k in csr._plans if isinstance(k, tuple) and k[0] == "list"]  # noqa: E731
    out = torch.full_like(X, float("nan"))
    propagate(csr, X, 2, out=out)  # records
    torch.cuda.synchronize()
    assert len(lists()) == 1 and ("groups", 2, 8) in csr._plans
    first = out.clone()
    assert bits_equal(first.cpu().numpy(),
                      propagate(csr, X, 2, hop_hook=lambda *a: None).cpu().numpy())
    X.copy_(torch.flip(X, dims=[0]) * 0.5)
    want = propagate(csr, X, 2, hop_hook=lambda *a: None).cpu().numpy()  # the hop loop
    propagate(csr, X, 2, out=out)  # replays
    torch.cuda.synchronize()
    assert len(lists()) == 1
    assert bits_equal(out.cpu().numpy(), want)
    assert not bits_equal(out.cpu().numpy(), first.cpu().numpy())


@pytest.mark.parametrize("F", [602, 64])
def test_accumulate_launch_light_count(oracle, prop_mod, F):
    """Groups >= 1 are empty for all but the first 5 rows: the accumulate
    launch's light item count (from the plan's fourth count) is the rows of
    the group that have nonzeros and are not heavy; the hop stays bit-exact
    (64 floats: the multi-row kernel, whose accumulate launch stops at that
    count; 602: the one-row kernel, which is given it and keeps row order)."""
    from sgc_amd.propagate import DeviceCSR, spmm
    n = 400
    rng = np.random.default_rng(F)
    rows = []
    for r in range(n):
        if r == 0:  # long enough to be a heavy row in both groups
            cols = np.sort(rng.choice(n, size=360, replace=False))
        elif r < 5:  # a few nonzeros on both sides of the cut
            cols = np.sort(np.concatenate([rng.choice(n // 2, size=3 + r, replace=False),
                                           n // 2 + rng.choice(n // 2, size=2 + r, replace=False)]))
        elif r % 7 == 0:
            cols = np.empty(0, np.int64)
        else:  # group 0's columns only
            cols = np.sort(rng.choice(n // 2, size=1 + r % 11, replace=False))
        rows.append((cols, rng.standard_normal(len(cols))))
    rp, ci, va = _csr_from_rows(rows)
    prop_mod.COLUMN_GROUPS, prop_mod.GROUP_WHOLE_ROWS = 2, 0
    csr = DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)
    X = rng.standard_normal((n, F)).astype(np.float32)
    out = torch.full((n, F), 777.0, dtype=torch.float32, device=DEV)
    spmm(csr, torch.from_numpy(X).to(DEV), out=out)
    torch.cuda.synchronize()
    assert bits_equal(out.cpu().numpy(), oracle.spmm_csr(rp, ci, va, X, 0, n))
    g0, g1 = csr.column_groups(2, 0)
    want_rp, _, _ = _split_host_whole(rp, ci, va, n, 2, 0)
    for part, wrp in ((g0, want_rp[0]), (g1, want_rp[1])):
        pl = part.plan(0, n, None, None, F)  # the cached plan of the launch above
        deg = np.diff(wrp.astype(np.int64))
        assert pl.ordered and pl.n_nonempty == int((deg > 0).sum())
        assert pl.n_heavy == int((deg > pl.threshold).sum())
        assert pl.accumulate_light_items == int(((deg > 0) & (deg <= pl.threshold)).sum())
    pl1 = g1.plan(0, n, None, None, F)
    assert pl1.n_nonempty == 5 and pl1.n_heavy == 1 and pl1.accumulate_light_items == 4
