"""The IEEE-edge operands of tests/ieee_operands.py, on the host.

Four things, none of which needs a GPU:

* the operands meet their conditions -- every row-length class of the result
  holds -0.0, subnormals, +-inf and NaN while most of it stays finite and
  normal -- asserted on torch.spmm's own output, never on the code under test;
* the oracle (oracle/spmm_oracle.c), which the GPU tests compare with, equals
  torch.spmm on these operands at 1 and 4 threads;
* the library's host twin (spmm / propagate / sgc_precompute on CPU tensors)
  equals torch.spmm on them;
* numpy mutants of the chain -- a trailing zero-weight FMA, flush-to-zero, a
  first product by multiply, an unfused multiply-add, the reversed order --
  differ from the contract in every row class where they can act, and the
  zero-weight FMA differs in no element on randn / positive-S operands, which
  is why the rest of the suite cannot see it.
"""
import functools

import numpy as np
import pytest
import torch

import ieee_operands as io

N = 4096
F_COND = 130  # tiny, huge, deep-tiny and special columns all present several times


@pytest.fixture(scope="module", autouse=True)
def _lib_built():
    from sgc_amd import build
    build.build(verbose=False)


def _coo_tensor(rows, cols, vals, n=N):
    idx = torch.from_numpy(np.stack([np.asarray(rows, np.int64), np.asarray(cols, np.int64)]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(vals, np.float32)), (n, n))


def _csr_rows(g):
    return np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.row_ptr))


@functools.lru_cache(maxsize=None)
def torch_hops(kind, F, K=1, threads=1, coo=False):
    """torch.spmm applied K times on the uncoalesced COO (CSR order, or the
    shuffled one with duplicates): [X_1 .. X_K] as numpy arrays."""
    g = io.edge_graph(N, 0, kind)
    A = _coo_tensor(*io.edge_coo(N, 0, kind)) if coo else _coo_tensor(_csr_rows(g), g.col_idx, g.val)
    X = torch.from_numpy(io.edge_features(N, F, kind).copy())
    saved = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        out = []
        for _ in range(K):
            X = torch.spmm(A, X)
            out.append(X.numpy())
    finally:
        torch.set_num_threads(saved)
    return out


# ---- the operands meet their conditions (on torch.spmm's result) ---------------

def test_graph_shape():
    g = io.edge_graph(N)
    lens = np.diff(g.row_ptr)
    assert set(io.ROW_LENGTHS) | set(io.LONG_ROWS) == set(np.unique(lens).tolist())
    assert sorted(lens[g.long_rows].tolist()) == sorted(io.LONG_ROWS + (io.LONG_NEGATIVE,))
    rows = _csr_rows(g)
    same_row = rows[1:] == rows[:-1]
    assert np.all(np.diff(g.col_idx.astype(np.int64))[same_row] > 0)  # strictly ascending
    assert g.col_idx.min() >= 0 and g.col_idx.max() < N
    # one all-negative row per length from 1 up and a long one, |s| in [2^-8, 2^-2)
    assert sorted(lens[g.negative_rows].tolist()) == sorted(io.ROW_LENGTHS[1:] + (io.LONG_NEGATIVE,))
    neg = np.isin(rows, g.negative_rows)
    assert np.all((g.val[neg] <= -2.0 ** -8) & (g.val[neg] > -2.0 ** -2))
    # the mixed long rows meet special nodes exactly at the chosen positions
    special, placed, huge = io.hot_nodes(N)
    hot = np.zeros(N, bool)
    hot[special] = True
    for r, L, (pos, ids) in zip(g.long_rows, io.LONG_ROWS, placed):
        cols = g.col_idx[g.row_ptr[r]:g.row_ptr[r + 1]]
        assert np.array_equal(np.nonzero(hot[cols])[0], pos) and np.array_equal(cols[pos], ids)
        assert not huge[cols].any()
    assert {0, 63, 64, 239, 240, 479, 480, 3000} == set(placed[0][0].tolist())
    q = io.edge_graph(N, 0, "quiet")
    assert np.array_equal(q.col_idx, g.col_idx) and np.abs(q.val).max() < 1.0
    assert np.array_equal(q.val, g.val * np.float32(2.0 ** -9))


def test_wild_conditions_on_torch_spmm():
    """Every nonempty class and every long row: -0.0, subnormal, +inf, -inf and
    NaN all occur, NaN takes at most 5 %, finite normals at least 60 %.  A
    -0.0 needs every product of a chain to underflow to -0 (zero products give
    +0.0 from the +0.0 start), which a mixed-sign row of hundreds of nonzeros
    with |s| up to 2^9 does not do: among the long rows the all-negative one
    delivers it."""
    Y = torch_hops("wild", F_COND)[0]
    g = io.edge_graph(N)
    cen = io.census(Y, g.row_class)
    print({k: v for k, v in cen.items()})
    assert cen["empty"]["pos_zero"] == cen["empty"]["total"]
    for name in io.SHORT_CLASSES + io.MIXED_LONG + ("longneg",):
        c = cen[name]
        need = ["subnormal", "pos_inf", "neg_inf", "nan"]
        if name not in io.MIXED_LONG:
            need.append("neg_zero")
        for k in need:
            assert c[k] >= 1, (name, k, c)
        assert c["nan"] <= 0.05 * c["total"], (name, c)
        assert c["normal"] >= 0.60 * c["total"], (name, c)
    # the all-negative rows against the +2^-149 column: -0.0, every length
    col = int(np.nonzero(io.column_kinds(F_COND) == 3)[0][0])
    assert np.all(Y[g.negative_rows, col].view(np.uint32) == 0x80000000)


def test_quiet_conditions_on_torch_spmm():
    """No non-finite element after 3 hops; -0.0 and subnormals per class after
    hop 1 (the long rows: see test_wild_conditions_on_torch_spmm)."""
    hops = torch_hops("quiet", F_COND, K=3)
    assert all(np.isfinite(Y).all() for Y in hops)
    g = io.edge_graph(N, 0, "quiet")
    cen = io.census(hops[0], g.row_class)
    for name in io.SHORT_CLASSES + io.MIXED_LONG + ("longneg",):
        assert cen[name]["subnormal"] >= 1, (name, cen[name])
        if name not in io.MIXED_LONG:
            assert cen[name]["neg_zero"] >= 1, (name, cen[name])
    assert io.census(hops[2], g.row_class)["17-64"]["normal"] > 0


def test_x86_nan_patterns_information():
    """Printed only: the NaN patterns torch.spmm produces here (the rule does
    not compare payload or sign)."""
    print("torch.spmm NaN patterns on the host:", io.nan_patterns(torch_hops("wild", F_COND)[0]))


# ---- the oracle equals the reference -------------------------------------------

@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("F", [33, F_COND])
def test_oracle_equals_torch_spmm(oracle, F, threads):
    g = io.edge_graph(N)
    X = io.edge_features(N, F, "wild")
    want = torch_hops("wild", F, 1, threads)[0]
    io.compare(oracle.spmm_csr(g.row_ptr, g.col_idx, g.val, X), want, "spmm_csr")
    io.compare(oracle.spmm_csr(g.row_ptr, g.col_idx, g.val, X, 100, 3000), want[100:3000], "rows")
    r, c, v = io.edge_coo(N)
    want_coo = torch_hops("wild", F, 1, threads, True)[0]
    io.compare(oracle.spmm_coo(N, r, c, v, X), want_coo, "spmm_coo")
    rp, ci, va = oracle.coo_to_csr(N, N, r, c, v)
    io.compare(oracle.spmm_csr(rp, ci, va, X), want_coo, "coo_to_csr + spmm_csr")
    # the duplicates and the shuffle change results: the COO case is its own case
    assert io.mismatches(want_coo, want).any()


@pytest.mark.parametrize("threads", [1, 4])
def test_oracle_propagate_equals_torch_spmm(oracle, threads):
    g = io.edge_graph(N, 0, "quiet")
    X = io.edge_features(N, 65, "quiet")
    want = torch_hops("quiet", 65, 3, threads)
    for K in (1, 3):
        io.compare(oracle.propagate(g.row_ptr, g.col_idx, g.val, X, K), want[K - 1], f"K={K}")
    gw = io.edge_graph(N)
    Xw = io.edge_features(N, 33, "wild")
    A = _coo_tensor(_csr_rows(gw), gw.col_idx, gw.val)
    two = torch.spmm(A, torch.spmm(A, torch.from_numpy(Xw.copy()))).numpy()
    io.compare(oracle.propagate(gw.row_ptr, gw.col_idx, gw.val, Xw, 2), two, "wild K=2")


# ---- the host twin -------------------------------------------------------------

@pytest.mark.parametrize("threads", [1, 3, 8])
def test_cpu_twin_one_hop_wild(threads):
    """spmm() on CPU tensors: the whole range, row ranges, ACCUMULATE over
    column splits (out starting as NaN), the shuffled COO with duplicates."""
    from sgc_amd.propagate import SPMM_ACCUMULATE, DeviceCSR, spmm
    g = io.edge_graph(N)
    F = 65
    want = torch_hops("wild", F)[0]
    X = torch.from_numpy(io.edge_features(N, F, "wild").copy())
    saved = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        csr = DeviceCSR.from_host_arrays(g.row_ptr, g.col_idx, g.val, device="cpu")
        io.compare(spmm(csr, X).numpy(), want, "spmm")
        for r0, r1 in ((0, 1), (5, 2300), (586, 587), (4000, N)):
            out = torch.full((r1 - r0, F + 7), float("nan"))
            spmm(csr, X, r0, r1, out=out[:, :F])
            io.compare(out[:, :F].numpy(), want[r0:r1], f"rows {r0}:{r1}")
            assert torch.isnan(out[:, F:]).all()
        for bounds in ([0, 700, 1100, 1600, N], [0, 5, N]):
            out = torch.full((N, F), float("nan"))
            for i, part in enumerate(io.column_groups(g, bounds)):
                sub = DeviceCSR.from_host_arrays(*part, n_cols=N, device="cpu")
                spmm(sub, X, out=out, flags=SPMM_ACCUMULATE if i else 0)
            io.compare(out.numpy(), want, f"accumulate {bounds}")
        adj = _coo_tensor(*io.edge_coo(N))
        io.compare(spmm(DeviceCSR.from_torch(adj), X).numpy(),
                   torch_hops("wild", F, coo=True)[0], "shuffled COO")
    finally:
        torch.set_num_threads(saved)


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_cpu_twin_three_hops_quiet(threads):
    """propagate() and sgc_precompute (the ingest's sort of the shuffled COO
    with duplicates) on CPU tensors, K = 3."""
    from sgc_amd.propagate import DeviceCSR, propagate
    from sgc_amd.utils import sgc_precompute
    g = io.edge_graph(N, 0, "quiet")
    F = 33
    X = torch.from_numpy(io.edge_features(N, F, "quiet").copy())
    saved = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        csr = DeviceCSR.from_host_arrays(g.row_ptr, g.col_idx, g.val, device="cpu")
        io.compare(propagate(csr, X, 3).numpy(), torch_hops("quiet", F, 3)[2], "propagate")
        out, _ = sgc_precompute(X, _coo_tensor(*io.edge_coo(N, 0, "quiet")), 3)
        io.compare(out.numpy(), torch_hops("quiet", F, 3, coo=True)[2], "sgc_precompute")
    finally:
        torch.set_num_threads(saved)


# ---- the comparison rule and the numpy chain -----------------------------------

def test_compare_rule():
    nan2 = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    a = np.array([[1.0, -0.0, np.nan, np.inf]], np.float32)
    io.compare(a, a.copy())
    io.compare(np.array([[1.0, -0.0, nan2, np.inf]], np.float32), a)  # payload and sign free
    for bad in ([1.0, 0.0, np.nan, np.inf], [1.0, -0.0, np.nan, -np.inf], [1.0, -0.0, 3.0, np.inf],
                [np.nan, -0.0, np.nan, np.inf], [np.float32(1.0) + np.float32(2.0 ** -23), -0.0,
                                                 np.nan, np.inf]):
        with pytest.raises(AssertionError):
            io.compare(np.array([bad], np.float32), a)
    t = torch.tensor([[1.0, -0.0, float("nan")]], dtype=torch.bfloat16)
    io.compare(t, t.clone())
    with pytest.raises(AssertionError):
        io.compare(torch.tensor([[1.0, 0.0, float("nan")]], dtype=torch.bfloat16), t)


def test_fma32_is_one_rounding():
    """fma32 against exact integer arithmetic on random and on halfway cases."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a = io._pow2_values(rng, 4000, -20, 20)
    b = io._pow2_values(rng, 4000, -20, 20)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)  # near cancellation
    c[::2] = io._pow2_values(rng, 2000, -30, 30)
    # halfway: a * b = 1 + 2^-23 + 2^-46 exactly, c a tiny push either way
    a[:4] = np.float32(1 + 2.0 ** -23)
    b[:4] = np.float32(1 + 2.0 ** -23)
    c[:4] = np.array([2.0 ** -24 - 2.0 ** -23, -2.0 ** -60, 2.0 ** -60, -2.0 ** -23 + 2.0 ** -24],
                     np.float32)
    got = io.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = Fraction(float(got[i]))  # the defining property: no float32 is nearer
        for nb in (np.nextafter(got[i], np.float32(np.inf)), np.nextafter(got[i], np.float32(-np.inf))):
            assert abs(g - exact) <= abs(Fraction(float(nb)) - exact), (i, a[i], b[i], c[i], got[i])


@functools.lru_cache(maxsize=None)
def _mutant_setup():
    from oracle import oracle as o
    o.build()
    g = io.edge_graph(N)
    X = io.edge_features(N, F_COND, "wild")
    return g, X, o.spmm_csr(g.row_ptr, g.col_idx, g.val, X)


def test_numpy_chain_equals_oracle():
    g, X, want = _mutant_setup()
    io.compare(io.chain(g.row_ptr, g.col_idx, g.val, X), want, "numpy chain")


def _hit_classes(mutant):
    g, X, want = _mutant_setup()
    bad = io.mismatches(io.chain(g.row_ptr, g.col_idx, g.val, X, mutant), want)
    hit = {io.CLASS_NAMES[c]: int(bad[g.row_class == c].sum()) for c in range(len(io.CLASS_NAMES))}
    print(mutant, hit)
    assert hit["empty"] == 0
    return hit


@pytest.mark.parametrize("mutant", ["zero_fma", "ftz", "unfused", "reversed"])
def test_mutant_caught_in_every_class(mutant):
    """Each of these can act on every row with nonzeros (a reversed chain on
    rows of at least two: the class 1-4 holds lengths 2, 3 and 4)."""
    hit = _hit_classes(mutant)
    for name in io.SHORT_CLASSES + io.MIXED_LONG + ("longneg",):
        assert hit[name] > 0, (mutant, name, hit)


def test_mutant_first_product_by_multiply():
    """A multiply in place of fma(s, x, +0.0) differs only while the chain is
    still a zero: where every product is -0 (negative s against the +0 column)
    the contract gives +0.0 and the mutant -0.0.  That is every class with an
    all-negative row; a mixed-sign long row leaves zero at its first normal
    product."""
    hit = _hit_classes("mul_first")
    for name in io.SHORT_CLASSES + ("longneg",):
        assert hit[name] > 0, (name, hit)


def test_zero_weight_fma_invisible_on_ordinary_operands():
    """The same graph with positive S in (0, 1] and X ~ N(0, 1) -- the operands
    of the rest of the suite: the trailing zero-weight FMA changes no element."""
    g = io.edge_graph(N)
    rng = np.random.default_rng(3)
    val = (1.0 - rng.random(g.val.size)).astype(np.float32)
    X = rng.standard_normal((N, 33)).astype(np.float32)
    plain = io.chain(g.row_ptr, g.col_idx, val, X)
    assert not io.mismatches(io.chain(g.row_ptr, g.col_idx, val, X, "zero_fma"), plain).any()
    assert io.mismatches(io.chain(g.row_ptr, g.col_idx, val, X, "reversed"), plain).any()


def test_big_graph_builds_quickly():
    """The million-row operands are vectorised: seconds, not minutes."""
    import time
    t0 = time.perf_counter()
    b = io.big_graph(1 << 20)
    X = io.edge_features(1 << 20, 5, "wild")
    secs = time.perf_counter() - t0
    lens = np.diff(b.row_ptr)
    assert b.n == 1 << 20 and X.shape == (1 << 20, 5)
    assert lens.max() == 3001 and (lens == 3001).sum() == 3 and ((lens >= 65) & (lens <= 300)).sum() == 300
    rows = np.repeat(np.arange(b.n), lens)
    assert np.all(np.diff(b.col_idx.astype(np.int64))[rows[1:] == rows[:-1]] > 0)
    assert b.col_idx.min() >= 0 and b.col_idx.max() < b.n
    assert secs < 20, secs


# ---- 16-bit features: the conditions on the emulation ---------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_x16_conditions_on_the_emulation(oracle, dtype):
    """The operands at a 16-bit format's own exponents, through the definition
    X_{k+1} = fp32_spmm(S, X_k.float()).to(T) (emulate() of test_gpu_x16.py).
    "wild": every short class and the long all-negative row hold -0.0, a 16-bit
    subnormal, +-inf and NaN; the mixed long rows +-inf and NaN (no 16-bit X is
    below 2^-133 / 2^-24, so their sums stay normal); NaN at most 5 %, normals at
    least 60 %.  "quiet": finite for three hops, -0.0 and subnormals after one."""
    from test_gpu_x16 import emulate
    g = io.edge_graph(N)
    csr = (g.row_ptr, g.col_idx, g.val)
    cen = io.census16(emulate(oracle, csr, io.edge_features16(N, F_COND, "wild", dtype), 1),
                      g.row_class)
    for name in io.SHORT_CLASSES + io.MIXED_LONG + ("longneg",):
        c = cen[name]
        need = ["pos_inf", "neg_inf", "nan"]
        if name not in io.MIXED_LONG:
            need += ["neg_zero", "subnormal"]
        for k in need:
            assert c[k] >= 1, (dtype, name, k, c)
        assert c["nan"] <= 0.05 * c["total"] and c["normal"] >= 0.60 * c["total"], (dtype, name, c)
    q = io.edge_graph(N, 0, "quiet")
    qcsr = (q.row_ptr, q.col_idx, q.val)
    Xq = io.edge_features16(N, F_COND, "quiet", dtype)
    assert torch.isfinite(emulate(oracle, qcsr, Xq, 3).float()).all()
    cen = io.census16(emulate(oracle, qcsr, Xq, 1), q.row_class)
    for name in io.SHORT_CLASSES + ("longneg",):
        assert cen[name]["neg_zero"] >= 1 and cen[name]["subnormal"] >= 1, (dtype, name, cen[name])
