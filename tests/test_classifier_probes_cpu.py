"""CPU checks of tests/classifier_probes.py: the numpy model of the split-bf16
scheme, the probes' own data, and the label-check cache.

This file is why the bounds of tests/test_gpu_classifier_exact.py are not
guesses: on exactly the single-term data those tests feed the kernels, the
intact six-product scheme stays inside 2^-22 and every scheme with one product
missing (or one piece misread) leaves it on most elements -- a subtly wrong
kernel would fail there.
"""
import numpy as np
import pytest
import torch

import classifier_probes as cp


def _single_term_pairs():
    """The (x, w) pairs of every single-term forward case of the GPU file."""
    xs, ws = [], []
    for (K, C) in cp.SINGLE_TERM_SHAPES:
        M = 2 * K + 1
        X, W, x, ref = cp.single_term_forward(M, K, C, seed=cp.single_term_seed(M, K, C))
        rows = torch.arange(M)
        xs.append(x[:, None].expand(M, C).reshape(-1))
        ws.append(W[:, rows % K].t().reshape(-1))
        # the generator's reference is the fp64 product of the pair
        assert torch.equal(ref.reshape(-1), xs[-1].double() * ws[-1].double())
        # and X holds exactly one value per row, at column m mod K
        assert torch.equal((X != 0).sum(1), torch.ones(M, dtype=torch.int64))
        assert torch.equal(X[rows, rows % K], x)
    return torch.cat(xs).numpy(), torch.cat(ws).numpy()


def test_split3_is_exact():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([cp.full_mantissa(g, (65536,)),
                   cp.full_mantissa(g, (4096,), emin=-100, emax=100),
                   torch.tensor([0.0, 1.0, -1.0, 255.0, 1023.0, 131071.0, 3.0e38, 1.0 + 2.0 ** -23]),
                   torch.randn(4096, generator=g)]).numpy()
    h, m, lo = cp.split3(x)
    for p in (h, m, lo):  # each piece is a bf16 value: low 16 bits clear
        assert not (p.view(np.uint32) & 0xFFFF).any()
    # h + m + l == x, with every partial sum exact
    assert np.array_equal((h.astype(np.float64) + m) + lo, x.astype(np.float64))
    assert np.array_equal((h + m) + lo, x)
    # RNE to bf16, against torch's own conversion
    assert np.array_equal(h, torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    # the pieces shrink as split_bf16.h says: |m| <= 2^-8 |h|, |l| <= 2^-8 |m|
    assert (np.abs(m) <= 2.0 ** -8 * np.abs(h)).all()
    assert (np.abs(lo) <= 2.0 ** -8 * np.abs(m)).all()


def test_intact_model_within_bound_on_probe_data():
    x, w = _single_term_pairs()
    ref = x.astype(np.float64) * w.astype(np.float64)
    err = cp.rel_err(cp.split_product_model(x, w), ref)
    # derived: 2^-24 for the final add, < 2^-24 for the dropped ml, lm, ll
    assert err.max() <= 2.0 * 2.0 ** -24, err.max() * 2.0 ** 24
    assert err.max() <= cp.SPLIT_BOUND
    # the fp32 kernels' single product: one rounding
    err32 = cp.rel_err(x * w, ref)
    assert err32.max() <= 2.0 ** -24 < cp.FP32_BOUND


@pytest.mark.parametrize("mutant", list(cp.PRODUCTS) + ["mm_as_ml"])
def test_every_mutant_leaves_the_bound(mutant):
    x, w = _single_term_pairs()
    ref = x.astype(np.float64) * w.astype(np.float64)
    if mutant == "mm_as_ml":
        got = cp.split_product_model(x, w, mm_as_ml=True)
    else:
        got = cp.split_product_model(x, w, drop=mutant)
    err = cp.rel_err(got, ref)
    outside = float((err > cp.SPLIT_BOUND).mean())
    assert outside >= 0.5, (mutant, outside, err.max() * 2.0 ** 24)


def test_mutants_fail_the_gpu_check_per_case():
    """check_single_term, the GPU tests' own verdict, on the model's output in
    place of a kernel's: intact passes, each mutant fails, for every single-
    term forward and backward case."""
    for (K, C) in cp.SINGLE_TERM_SHAPES:
        M = 2 * K + 1
        X, W, x, ref = cp.single_term_forward(M, K, C, seed=cp.single_term_seed(M, K, C))
        rows = torch.arange(M)
        xe = x[:, None].expand(M, C).numpy()
        we = W[:, rows % K].t().numpy()
        worst, ok = cp.check_single_term(torch.from_numpy(cp.split_product_model(xe, we)), ref,
                                         cp.SPLIT_BOUND)
        assert ok and worst <= 2.0, worst
        for mutant in cp.PRODUCTS:
            got = torch.from_numpy(cp.split_product_model(xe, we, drop=mutant))
            assert not cp.check_single_term(got, ref, cp.SPLIT_BOUND)[1], mutant
        got = torch.from_numpy(cp.split_product_model(xe, we, mm_as_ml=True))
        assert not cp.check_single_term(got, ref, cp.SPLIT_BOUND)[1]
    for (M, K, C, r0) in cp.single_term_backward_cases():
        X, dY, dYb, wref, wbref, bref = cp.single_term_backward(
            M, K, C, r0, seed=cp.single_term_seed(M, K, C) + r0)
        # the references against the plain fp64 products
        assert torch.equal(wref, dY.double().t() @ X.double())
        assert torch.equal(wbref, dYb.double().t() @ X.double())
        assert torch.equal(bref.double(), dYb.double().sum(0))
        assert int((wref != 0).sum()) == C * (min(r0 + K, M) - r0)
        # a kernel that drops a product: model it on the non-zero elements
        r1 = min(r0 + K, M)
        xe = X[r0:r1].sum(1)[None, :].expand(C, r1 - r0).numpy()  # the one value per row
        ge = dY[r0:r1].t().numpy()
        for mutant in (None,) + cp.PRODUCTS:
            got = torch.zeros_like(wref)
            got[:, torch.arange(r0, r1) % K] = torch.from_numpy(
                cp.split_product_model(ge, xe, drop=mutant)).double()
            ok = cp.check_single_term(got, wref, cp.SPLIT_BOUND)[1]
            assert ok == (mutant is None), (M, K, C, r0, mutant)
        # a stray non-zero where zero is expected fails whatever its size
        if (wref == 0).any():
            got = wref.clone()
            got[wref == 0] = 1e-30
            assert not cp.check_single_term(got, wref, cp.SPLIT_BOUND)[1]


def test_integer_generators_meet_their_bound():
    """Every integer case of the GPU file: the generator's own assertion
    (sum |x||w| + |b| < 2^24 over the bf16 pieces' magnitudes) holds, the
    values are integers, and the intended bf16 pieces are populated."""
    def pieces(t):
        h, m, lo = cp.split3(t.numpy())
        return bool(m.any()), bool(lo.any())

    for (M, K, C, ld_extra, bits, wide, kernels, auto) in cp.FORWARD_CASES:
        X, W, b = cp.integer_operands(M, K, C, bits, seed=cp.case_seed(M, K, C), wide=wide)
        for t in (X, W, b):
            assert t.dtype == torch.float32 and torch.equal(t, t.round())
        assert cp.integer_bound(X, W, b) < cp.EXACT_LIMIT
        wd = X if wide == "x" else W
        assert pieces(wd) == {8: (False, False), 10: (True, False), 18: (True, True)}[bits]
        # exact in fp32 in any order: forwards, backwards and fp64 agree
        ref = torch.nn.functional.linear(X.double(), W.double(), b.double())
        assert torch.equal(torch.nn.functional.linear(X, W, b).double(), ref)
        assert torch.equal((X.flip(1) @ W.flip(1).t() + b).double(), ref)
    for (M, K, C, ldx_extra, ldd_extra, bits, wide, kernels) in cp.BACKWARD_CASES:
        X, dY = cp.integer_operands(M, K, C, bits, seed=cp.case_seed(M, K, C), backward=True,
                                    wide=wide)
        assert torch.equal(X, X.round()) and torch.equal(dY, dY.round())
        wd = X if wide == "x" else dY
        assert pieces(wd) == {8: (False, False), 10: (True, False), 18: (True, True)}[bits]
        ref = dY.double().t() @ X.double()
        assert torch.equal((dY.t() @ X).double(), ref)
        assert float(ref.abs().max()) < cp.EXACT_LIMIT
    with pytest.raises(AssertionError):  # 18-bit operands refuse long dot products
        cp.integer_operands(8, 41, 4, 18, seed=0)


def test_case_tables_cover_the_issue_sets():
    """The hand-picked shapes draw on every size the issue lists."""
    fm = {c[0] for c in cp.FORWARD_CASES}
    fk = {c[1] for c in cp.FORWARD_CASES}
    fc = {c[2] for c in cp.FORWARD_CASES}
    assert fm == {1, 15, 17, 33, 129, 257, 4099, 70000}
    assert fk == {1, 3, 31, 33, 63, 65, 130, 333, 602}
    assert fc == {1, 15, 16, 17, 41, 42, 48, 49, 64, 65, 70, 129}
    assert {c[3] for c in cp.FORWARD_CASES} == {0, 1, 2, 6}
    assert any("p" in c[6] and c[2] == 65 for c in cp.FORWARD_CASES)  # split, 2nd block of 1
    assert any("p" in c[6] and c[2] == 70 for c in cp.FORWARD_CASES)  # split, 2nd block of 6
    assert {c[1] for c in cp.BACKWARD_CASES} == {1, 3, 34, 63, 64, 65, 130, 602}
    assert {c[2] for c in cp.BACKWARD_CASES} == {1, 2, 16, 17, 32, 33, 41, 48, 49, 64}
    assert {33, 6145, 12321} <= {c[0] for c in cp.BACKWARD_CASES}
    for kind in "cfs":
        assert any(kind in c[7] for c in cp.BACKWARD_CASES)


def test_label_check_is_per_tensor_object():
    """models._check_labels: one check per labels tensor and version (the
    LBFGS closures pass the same tensor every call), but never a pass carried
    over to ANOTHER tensor at the same address -- keyed on data_ptr(), a new
    labels tensor in a reused block skipped validation."""
    from sgc_amd import models
    arr = np.arange(64, dtype=np.int64) % 5
    y1 = torch.from_numpy(arr)
    models._check_labels(y1, 5, -100)
    entry = models._checked_labels[id(y1)]
    models._check_labels(y1, 5, -100)
    assert models._checked_labels[id(y1)] is entry  # cached: no second check
    # a second tensor over the same memory (same data_ptr, same version, same
    # length) holding an out-of-range label must be checked, and fail
    arr[3] = 9
    y2 = torch.from_numpy(arr)
    assert y2.data_ptr() == y1.data_ptr() and y2._version == y1._version
    with pytest.raises(IndexError, match="out of bounds"):
        models._check_labels(y2, 5, -100)
    # an in-place update of a checked tensor is checked again
    y3 = torch.arange(64) % 5
    models._check_labels(y3, 5, -100)
    y3[7] = -1
    with pytest.raises(IndexError, match="out of bounds"):
        models._check_labels(y3, 5, -100)
    y3[7] = -100  # ignore_index passes
    models._check_labels(y3, 5, -100)
    with pytest.raises(IndexError):  # ... but not under another ignore_index
        models._check_labels(y3, 5, -1)
    # the freed-and-reallocated form: whether or not the allocator reuses the
    # block, the new tensor is validated
    n = len(models._checked_labels)
    good = torch.zeros(4160, dtype=torch.int64)
    models._check_labels(good, 5, -100)
    assert len(models._checked_labels) == n + 1
    del good
    assert len(models._checked_labels) == n  # the entry dies with its tensor
    bad = torch.full((4160,), 7, dtype=torch.int64)
    with pytest.raises(IndexError, match="out of bounds"):
        models._check_labels(bad, 5, -100)
