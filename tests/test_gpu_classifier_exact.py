"""The classifier kernels (linear.hip, xent.hip, loss.hip) against fp64 torch
with no tolerance to hide in: integer operands (every kernel must be bit-exact,
at every shape edge), single-term operands (one product per output: 2^-23
relative for the fp32 kernels, 2^-22 for the split-bf16 ones -- bounds that
tests/test_classifier_probes_cpu.py shows every one-product-missing scheme
breaks), softmax rows far from the origin, and non-finite features in the
weight backward.  Operands: tests/classifier_probes.py.
"""
import functools

import pytest
import torch

import classifier_probes as cp

pytestmark = pytest.mark.gpu

DEV = "cuda"
F_ = torch.nn.functional


def _lib():
    from sgc_amd import _lib
    return _lib, _lib.load()


class _Tuning:
    """Set tuning knobs for a block and restore the previous values after it."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        _l, lib = _lib()
        self.prev = {k: lib.sgc_get_tuning(k.encode()) for k in self.knobs}
        for k, v in self.knobs.items():
            _l.check(lib.sgc_set_tuning(k.encode(), v), f"set_tuning {k}")
        return self

    def __exit__(self, *exc):
        _l, lib = _lib()
        for k, v in self.prev.items():
            lib.sgc_set_tuning(k.encode(), v)
        return False


_FWD_NAMES = {"t": "linear_kernel", "s": "linear_stream_kernel", "p": "linear_split_kernel"}
_BWD_NAMES = {"c": "xent_dw_cols_kernel", "f": "xent_dw_kernel", "s": "xent_dw_split_kernel"}


def _forward_configs(kernels):
    """(label, knobs, expected kernel) of every forward kernel a case names."""
    out = []
    if "t" in kernels:
        out += [(f"tile/{nb}", dict(linear_kernel=1, tile_buffers=nb), "t") for nb in (1, 2)]
    if "s" in kernels:
        out += [(f"stream/{ck}", dict(linear_kernel=2, linear_ck=ck), "s") for ck in (32, 64)]
    if "p" in kernels:
        out += [("split", dict(linear_kernel=5), "p")]
    return out


def _assert_forward_kernel(lib, _l, M, K, C, Xd, want):
    name = lib.sgc_linear_kernel_name(M, K, Xd.stride(0), C, _l.ptr(Xd)).decode()
    assert name.split(" ")[0] == want, (name, want)


# ---- 1. integer operands, bit-exact forward ------------------------------------

@pytest.mark.parametrize("M,K,C,ld_extra,bits,wide,kernels,auto", cp.FORWARD_CASES)
def test_forward_integer_bit_exact(M, K, C, ld_extra, bits, wide, kernels, auto):
    """Integer operands (every product and partial sum exact in fp32): each
    forward kernel the case names -- the LDS tile with one and two images,
    the fp32 streaming kernel at 32- and 64-k chunks with 16-B or 8-B row
    loads, the split-bf16 kernel, the automatic choice at M >= 4096 -- equals
    fp64 torch bit for bit, with a bias and without.  X is a column slice of a
    tensor whose padding holds NaN; the result goes into a column slice of a
    NaN-filled tensor whose padding must stay NaN.  Up to 64 classes the fused
    step's logits (xent_fwd_kernel, one and two images) are held to the same."""
    from sgc_amd.propagate import linear, linear_xent
    _l, lib = _lib()
    X, W, b = cp.integer_operands(M, K, C, bits, seed=cp.case_seed(M, K, C), wide=wide)
    ref = F_.linear(X.double(), W.double(), b.double()).float()  # exact, so the cast is
    ref_nb = F_.linear(X.double(), W.double()).float()
    Xd, _ = cp.nan_padded(X, ld_extra, DEV)
    Wd, bd = W.to(DEV), b.to(DEV)
    pad = 3

    def run(label):
        for bias, want in ((bd, ref), (None, ref_nb)):
            whole = torch.full((M, C + pad), float("nan"), device=DEV)
            got = linear(Xd, Wd, bias, out=whole[:, :C])
            assert got.data_ptr() == whole.data_ptr()
            assert torch.equal(whole[:, :C].cpu(), want), (label, bias is not None)
            assert torch.isnan(whole[:, C:]).all(), label

    configs = _forward_configs(kernels)
    if auto is not None:
        assert M >= 4096
        configs.append(("auto", dict(linear_kernel=0), None))
    for label, knobs, kind in configs:
        with _Tuning(**knobs):
            _assert_forward_kernel(lib, _l, M, K, C, Xd, _FWD_NAMES[kind] if kind else auto)
            run(label)
    if C <= 64:
        y = (torch.arange(M) % C).to(DEV)
        for nb in (1, 2):
            with _Tuning(tile_buffers=nb):
                logits = linear_xent(Xd, Wd, bd, y, want_logits=True)[3]
                assert torch.equal(logits.cpu(), ref), ("xent logits", nb)


# ---- 2. integer operands, bit-exact backward -----------------------------------

@pytest.mark.parametrize("M,K,C,ldx_extra,ldd_extra,bits,wide,kernels", cp.BACKWARD_CASES)
def test_backward_integer_bit_exact(M, K, C, ldx_extra, ldd_extra, bits, wide, kernels):
    """dW = dY^T X and db = sum dY on integer operands: backward_kernel 0, 1,
    2 and 3 -- the split-bf16 column blocks, the fp32 slabs, the split-bf16
    slabs, each named before it runs -- equal fp64 torch bit for bit; X and dY
    are column slices of tensors whose padding holds NaN; want_bias=False gives
    the same dW.  Which loop edge each M, K and C hits: classifier_probes.
    BACKWARD_CASES."""
    from sgc_amd.propagate import linear_backward
    _l, lib = _lib()
    X, dY = cp.integer_operands(M, K, C, bits, seed=cp.case_seed(M, K, C), backward=True,
                                wide=wide)
    wref = (dY.double().t() @ X.double()).float()
    bref = dY.double().sum(0).float()
    Xd, _ = cp.nan_padded(X, ldx_extra, DEV)
    Gd, _ = cp.nan_padded(dY, ldd_extra, DEV)
    for kernel in (0, 1, 2, 3):
        with _Tuning(backward_kernel=kernel):
            name = lib.sgc_linear_backward_kernel_name(M, K, Xd.stride(0), C, _l.ptr(Xd)).decode()
            assert name.split(" ")[0] == _BWD_NAMES[kernels[kernel]], (kernel, name)
            dW, db = linear_backward(Xd, Gd)
            assert torch.equal(dW.cpu(), wref), (kernel, name)
            assert torch.equal(db.cpu(), bref), (kernel, name)
            dW2, none = linear_backward(Xd, Gd, want_bias=False)
            assert none is None and torch.equal(dW2, dW), (kernel, name)


# ---- 3. single-term probes, full mantissas -------------------------------------

@pytest.mark.parametrize("K,C", cp.SINGLE_TERM_SHAPES)
def test_forward_single_term(K, C):
    """Y[m, c] = x[m] * W[c, m mod K], one product of two full-mantissa values
    (M = 2 K + 1: every k position, rows wrap; no bias).  fp32 kernels: within
    2^-23 relative (one rounding of one product is 2^-24; adding zeros is
    exact).  Split-bf16 kernel: within 2^-22 (split_bf16.h: 2^-24 for the final
    add, below 2^-24 for the dropped ml, lm, ll products) -- a kernel that loses
    any one of the six products fails it (test_classifier_probes_cpu.py)."""
    from sgc_amd.propagate import linear
    _l, lib = _lib()
    M = 2 * K + 1
    X, W, x, ref = cp.single_term_forward(M, K, C, seed=cp.single_term_seed(M, K, C))
    Xd, _ = cp.nan_padded(X, 2 - K % 2, DEV)  # an even pitch for the streaming kernel
    Wd = W.to(DEV)
    for label, knobs, kind in _forward_configs("tsp"):
        with _Tuning(**knobs):
            _assert_forward_kernel(lib, _l, M, K, C, Xd, _FWD_NAMES[kind])
            Y = linear(Xd, Wd, None).cpu()
        bound = cp.SPLIT_BOUND if kind == "p" else cp.FP32_BOUND
        worst, ok = cp.check_single_term(Y, ref, bound)
        print(f"single-term forward K={K} C={C} {label}: max rel err {worst:.3f} x 2^-24")
        assert ok, (label, worst)


@pytest.mark.parametrize("M,K,C,r0", cp.single_term_backward_cases())
def test_backward_single_term(M, K, C, r0):
    """dY non-zero on K consecutive rows from r0 (first, middle, last and
    partial): each dW[c, k] is one product dY[m, c] * x[m] or exactly zero;
    with one element of dY per class db is that element, bit for bit.  Bounds
    as in the forward: 2^-23 for the fp32 slabs, 2^-22 for the two split-bf16
    kernels; expected zeros must be exactly zero."""
    from sgc_amd.propagate import linear_backward
    _l, lib = _lib()
    X, dY, dYb, wref, wbref, bref = cp.single_term_backward(
        M, K, C, r0, seed=cp.single_term_seed(M, K, C) + r0)
    Xd, _ = cp.nan_padded(X, 2 - K % 2, DEV)
    Gd, Gbd = dY.to(DEV), dYb.to(DEV)
    kinds = "cfsc"  # C <= 48, an even pitch and (below) an even K
    if K % 2:
        kinds = "cffc"
    for kernel in (0, 1, 2, 3):
        with _Tuning(backward_kernel=kernel):
            name = lib.sgc_linear_backward_kernel_name(M, K, Xd.stride(0), C, _l.ptr(Xd)).decode()
            assert name.split(" ")[0] == _BWD_NAMES[kinds[kernel]], (kernel, name)
            dW, _ = linear_backward(Xd, Gd)
            dWb, db = linear_backward(Xd, Gbd)
        bound = cp.FP32_BOUND if kinds[kernel] == "f" else cp.SPLIT_BOUND
        worst, ok = cp.check_single_term(dW.cpu(), wref, bound)
        worst_b, ok_b = cp.check_single_term(dWb.cpu(), wbref, bound)
        print(f"single-term backward M={M} K={K} C={C} r0={r0} {name.split(' ')[0]}: "
              f"max rel err {max(worst, worst_b):.3f} x 2^-24")
        assert ok and ok_b, (kernel, name, worst, worst_b)
        assert torch.equal(db.cpu(), bref), (kernel, name)


# ---- 4. softmax edges -----------------------------------------------------------

OFFSETS = (0.0, 1000.0, -1000.0, 30000.0, -30000.0)


@functools.lru_cache(maxsize=None)
def _softmax_rows(M, C):
    """{name: (logits [M, C] fp32, labels [M])}: the rows the softmax can get
    wrong -- far from the origin, saturated, flat."""
    g = torch.Generator().manual_seed(100 * M + C)
    base = torch.randn((M, C), generator=g) * 3
    y = torch.randint(0, C, (M,), generator=g)
    rows = {}
    for off in OFFSETS:
        rows[f"offset{off:+.0f}"] = (base + off, y)
    for lead in (200.0, 1.0e4):
        z = base.clone()
        top = torch.randint(0, C, (M,), generator=g)
        z[torch.arange(M), top] = base.max(1).values + lead
        rows[f"lead{lead:.0f}/label_on_it"] = (z, top)
        rows[f"lead{lead:.0f}/label_on_smallest"] = (z, z.argmin(1))
    rows["all_equal"] = (torch.full((M, C), 7.25), y)
    rows["all_equal_far"] = (torch.full((M, C), -30000.0), y)
    return rows


@pytest.mark.parametrize("C", [1, 3, 41, 64])
@pytest.mark.parametrize("M", [7, 1000])
def test_logits_cross_entropy_softmax_edges(M, C):
    """F.cross_entropy on SGCLogits (sgc_cross_entropy_f32 / _backward_f32)
    against fp64 torch on the same fp32 logits, at the project's tolerances
    (loss rtol 1e-5, atol 1e-6; gradient rtol 1e-4, atol 1e-7 for an incoming
    gradient of 1): a common offset of 0, +-1000, +-30000 (softmax does not
    depend on it; lse = m + log s rounded to ulp(|lse|) and then subtracted
    did: 9.5e-4 / M at 30000), one logit ahead by 200 and by 1e4 with the
    label on it and on the smallest logit, all logits equal; every seventh row
    ignore_index.  All results finite."""
    from sgc_amd.models import SGCLogits
    for name, (z, y0) in _softmax_rows(M, C).items():
        y = y0.clone()
        y[3::7] = -100
        ref_x = z.double().requires_grad_()
        ref = F_.cross_entropy(ref_x, y)
        ref.backward()
        zd = z.to(DEV).requires_grad_()
        loss = F_.cross_entropy(zd.as_subclass(SGCLogits), y.to(DEV))
        assert "LogitsCrossEntropy" in type(loss.grad_fn).__name__
        loss.backward()
        got_l, got_g = loss.detach().cpu().double(), zd.grad.cpu().double()
        assert torch.isfinite(got_l) and torch.isfinite(got_g).all(), name
        dl = float((got_l - ref.detach()).abs())
        dg = float((got_g - ref_x.grad).abs().max()) * M
        print(f"softmax edges M={M} C={C} {name}: |dloss| {dl:.3e}, max |dgrad| {dg:.3e} / M")
        torch.testing.assert_close(got_l, ref.detach(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}: {m}")
        torch.testing.assert_close(got_g, ref_x.grad, rtol=1e-4, atol=1e-7,
                                   msg=lambda m: f"{name}: {m}")
        assert (got_g[3::7] == 0).all()


@pytest.mark.parametrize("C", [1, 3, 41, 64])
@pytest.mark.parametrize("M", [7, 1000])
def test_fused_xent_softmax_edges(M, C):
    """The fused step (xent_fwd_kernel's softmax) on the same kinds of rows:
    the offset comes through the bias, the spread from scaled one-hot rows of
    X -- X[m] = a e_k gives logits a W[:, k] + b: k < 8 picks a 3 randn column,
    k >= 8 a column that is 1 at one class (scaled by 200 or 1e4: that class
    leads by as much), a zero row gives all logits equal.  The reference is
    fp64 cross-entropy of the kernel's own returned logits, so the rounding of
    the fp32 logits is not charged to the softmax: loss (rtol 1e-5, atol 1e-6)
    and db = sum_m G (rtol 1e-4, atol 1e-7: sum_m |G| <= 2) against it, dW
    against G_ref^T X in fp64 (rtol 1e-4, atol 1e-7 max|x|: |dW| <= 2 max|x|)."""
    from sgc_amd.propagate import linear_xent
    g = torch.Generator().manual_seed(7 * M + C)
    K = 16
    W = torch.zeros((C, K))
    W[:, :8] = torch.randn((C, 8), generator=g) * 3
    lead_cls = torch.randint(0, C, (8,), generator=g)
    W[lead_cls, torch.arange(8, 16)] = 1.0
    kind = torch.arange(M) % 5  # 0, 1: randn rows; 2: lead 200; 3: lead 1e4; 4: flat
    col = torch.where(kind < 2, torch.randint(0, 8, (M,), generator=g),
                      torch.randint(8, 16, (M,), generator=g))
    amp = torch.tensor([1.0, 1.0, 200.0, 1.0e4, 0.0])[kind]
    X = torch.zeros((M, K))
    X[torch.arange(M), col] = amp
    y_rand = torch.randint(0, C, (M,), generator=g)
    for off in OFFSETS:
        b = torch.full((C,), off)
        z0 = F_.linear(X.double(), W.double(), b.double())
        # labels: on the leading class, on the smallest logit, or anywhere
        y = torch.where(torch.arange(M) % 2 == 0, z0.argmax(1), z0.argmin(1))
        y = torch.where(kind < 2, y_rand, y)
        loss, dW, db, logits = linear_xent(X.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV),
                                           want_logits=True)
        for t in (loss, dW, db, logits):
            assert torch.isfinite(t).all(), off
        zk = logits.cpu().double()
        torch.testing.assert_close(zk, z0, rtol=1e-6, atol=0)  # one product + bias, rounded
        lref = F_.cross_entropy(zk, y)
        G = (torch.softmax(zk, 1) - F_.one_hot(y, C).double()) / M
        dl = float((loss.cpu().double() - lref).abs())
        ddb = float((db.cpu().double() - G.sum(0)).abs().max())
        ddw = float((dW.cpu().double() - G.t() @ X.double()).abs().max())
        print(f"fused softmax edges M={M} C={C} offset {off:+.0f}: |dloss| {dl:.3e}, "
              f"max |ddb| {ddb:.3e}, max |ddW| {ddw:.3e}")
        torch.testing.assert_close(loss.cpu().double(), lref, rtol=1e-5, atol=1e-6,
                                   msg=lambda m: f"offset {off}: {m}")
        torch.testing.assert_close(db.cpu().double(), G.sum(0), rtol=1e-4, atol=1e-7,
                                   msg=lambda m: f"offset {off}: {m}")
        wref = G.t() @ X.double()
        room = 1e-7 * X.abs().max(0).values.double()[None, :] + 1e-4 * wref.abs()
        over = (dW.cpu().double() - wref).abs() - room
        assert (over <= 0).all(), (off, float(over.max()))


# ---- 5. non-finite features in the weight backward -----------------------------

def test_backward_nonfinite_features():
    """The counterpart of test_linear_split_nonfinite_inside_k for dW: with
    +inf, -inf and NaN inside X's K range, the default backward (the split-
    bf16 column blocks: x - bf16(x) is inf - inf) gives NaN in those columns
    of dW for every class, where torch gives +-inf by dY's sign (NaN for the
    NaN); backward_kernel = 1 (fp32 MFMA slabs) reproduces torch's values
    there; every other column stays within the fp32 tolerance, and db (dY's
    column sums) is untouched, under both settings."""
    from sgc_amd.propagate import linear_backward
    _l, lib = _lib()
    M, K, C = 1000, 602, 41
    g = torch.Generator().manual_seed(11)
    X = torch.randn((M, K), generator=g)
    dY = torch.randn((M, C), generator=g) / M
    bad = {5: (100, float("inf")), 77: (3, float("-inf")), 500: (601, float("nan")),
           999: (0, float("inf"))}
    for r, (k, v) in bad.items():
        X[r, k] = v
    cols = torch.tensor(sorted(k for k, _ in bad.values()))
    good = torch.ones(K, dtype=torch.bool)
    good[cols] = False
    with torch.no_grad():
        wref = dY.double().t() @ X.double()
    bref = dY.double().sum(0)
    assert torch.isinf(wref[:, [0, 3, 100]]).all() and torch.isnan(wref[:, 601]).all()
    tol = 1e-5 * max(1e-3, wref[:, good].abs().max().item())
    Xd, Gd = X.to(DEV), dY.to(DEV)
    for kernel, want in ((0, "xent_dw_cols_kernel"), (1, "xent_dw_kernel")):
        with _Tuning(backward_kernel=kernel):
            name = lib.sgc_linear_backward_kernel_name(M, K, Xd.stride(0), C, _l.ptr(Xd)).decode()
            assert name.split(" ")[0] == want, name
            dW, db = linear_backward(Xd, Gd)
        dW, db = dW.cpu().double(), db.cpu().double()
        if kernel == 0:
            assert torch.isnan(dW[:, cols]).all()  # the deviation: NaN, not torch's +-inf
        else:
            torch.testing.assert_close(dW[:, cols], wref[:, cols], rtol=0, atol=0, equal_nan=True)
        torch.testing.assert_close(dW[:, good], wref[:, good], rtol=1e-4, atol=tol)
        torch.testing.assert_close(db, bref, rtol=1e-4, atol=1e-5 * bref.abs().max().item())


# ---- the label check belongs to the tensor, not to its address ------------------

def test_label_check_survives_block_reuse():
    """A labels tensor passes the range check once (the LBFGS closures); a NEW
    tensor of the same length that the allocator places in the freed one's
    block is checked again.  Keyed on data_ptr() it was not: its out-of-range
    label reached the kernel and the loss was NaN.  The test fails, never
    skips, if the block is not reused."""
    from sgc_amd import models
    from sgc_amd.models import SGCLogits
    n, C = 4160, 5  # 33,280 B: an unusual size, so the freed block is the best fit
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    x = torch.randn((n, C), device=DEV).as_subclass(SGCLogits)
    y = torch.randint(0, C, (n,), device=DEV)
    after = torch.empty(n, dtype=torch.int64, device=DEV)  # keeps y's block from merging
    assert torch.isfinite(F_.cross_entropy(x, y))
    entry = models._checked_labels[id(y)]
    assert entry[0]() is y
    assert torch.isfinite(F_.cross_entropy(x, y))
    assert models._checked_labels[id(y)] is entry  # cached: no second check
    freed = y.data_ptr()
    del y, entry
    torch.cuda.synchronize()
    y_bad = torch.full((n,), C + 2, dtype=torch.int64, device=DEV)
    assert y_bad.data_ptr() == freed, "the allocator did not reuse the freed labels block"
    assert y_bad._version == 0
    with pytest.raises(IndexError, match="out of bounds"):
        F_.cross_entropy(x, y_bad)
    del after
