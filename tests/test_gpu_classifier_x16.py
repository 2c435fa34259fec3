"""The classifier on 16-bit features (csrc/linear16.hip: linear_x16_kernel,
xent_dw_cols_x16_kernel) against fp64 torch on the exactly widened X: integer
operands bit for bit at every shape edge, single-term probes within 2^-23
(bf16 X) / 2^-22 (fp16 X) -- bounds every one-product-missing scheme breaks
(tests/test_classifier_x16_cpu.py) -- randn at the project's tolerance,
non-finite features, the module level and the pipeline.  X is always a column
slice of a NaN-padded 16-bit tensor, `out=` a slice of a NaN-filled tensor
whose padding must stay NaN.  Operands: tests/classifier_probes_x16.py.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import classifier_probes as cp
import classifier_probes_x16 as p16

pytestmark = pytest.mark.gpu

DEV = "cuda"
F_ = torch.nn.functional
DT = pytest.mark.parametrize("dtype", p16.DTYPES, ids=["bf16", "fp16"])
SGC_DT = {torch.bfloat16: 1, torch.float16: 2}
RANDN_SHAPES = [(1000, 602, 41, 2), (1000, 500, 3, 2), (999, 1433, 7, 1)]  # M, K, C, pad


def _lib():
    from sgc_amd import _lib
    return _lib, _lib.load()


def _fwd_name(Xd):
    _l, lib = _lib()
    M, K = Xd.shape
    return lambda C: lib.sgc_linear_x16_kernel_name(M, K, Xd.stride(0), C, _l.ptr(Xd),
                                                    SGC_DT[Xd.dtype]).decode().split(" ")[0]


def _bwd_name(Xd, C):
    _l, lib = _lib()
    M, K = Xd.shape
    return lib.sgc_linear_backward_x16_kernel_name(M, K, Xd.stride(0), C, _l.ptr(Xd),
                                                   SGC_DT[Xd.dtype]).decode().split(" ")[0]


def _linear_into_padded(Xd, Wd, bias, C, pad=3):
    """linear(..., out=slice of a NaN-filled tensor): the result, after
    checking that it went there and that the padding is still NaN."""
    from sgc_amd.propagate import linear
    whole = torch.full((Xd.shape[0], C + pad), float("nan"), device=DEV)
    got = linear(Xd, Wd, bias, out=whole[:, :C])
    assert got.data_ptr() == whole.data_ptr()
    assert torch.isnan(whole[:, C:]).all()
    return whole[:, :C].cpu()


# ---- 1. forward, integer operands, bit-exact ---------------------------------------

@DT
@pytest.mark.parametrize("M,K,C,pad,m_bf16,m_fp16,kernel", p16.FORWARD_CASES)
def test_forward_integer_bit_exact(dtype, M, K, C, pad, m_bf16, m_fp16, kernel):
    """Y = float(X) W^T + b on integer operands equals fp64 torch bit for bit,
    with a bias and without: the x16 kernel where it is named, the copy path
    at an odd pitch (no kernel named for the view), the upcast path where W's
    image exceeds LDS."""
    bits, wide = p16.mode_of((m_bf16, m_fp16), dtype)
    X, W, b = p16.integer_operands_x16(M, K, C, bits, cp.case_seed(M, K, C), dtype, wide=wide)
    ref = F_.linear(X.double(), W.double(), b.double()).float()  # exact, so the cast is
    ref_nb = F_.linear(X.double(), W.double()).float()
    Xd, _ = p16.nan_padded16(X, pad, DEV)
    Wd, bd = W.to(DEV), b.to(DEV)
    assert _fwd_name(Xd)(C) == kernel
    if kernel == "none" and Xd.stride(0) % 2:  # the layout alone: an even-pitch copy is covered
        from sgc_amd.propagate import _even_pitch_x16
        assert _fwd_name(_even_pitch_x16(Xd))(C) == "linear_x16_kernel"
    for bias, want in ((bd, ref), (None, ref_nb)):
        assert torch.equal(_linear_into_padded(Xd, Wd, bias, C), want), bias is not None


# ---- 2. backward, integer operands, bit-exact --------------------------------------

@DT
@pytest.mark.parametrize("M,K,C,ldx_pad,ldd_pad,m_bf16,m_fp16,kernel", p16.BACKWARD_CASES)
def test_backward_integer_bit_exact(dtype, M, K, C, ldx_pad, ldd_pad, m_bf16, m_fp16, kernel):
    """dW = dY^T float(X) and db = sum dY on integer operands equal fp64 torch
    bit for bit; want_bias=False gives the same dW; above 48 classes no kernel
    is named and the upcast path is as exact."""
    from sgc_amd.propagate import linear_backward
    bits, wide = p16.mode_of((m_bf16, m_fp16), dtype)
    X, dY = p16.integer_operands_x16(M, K, C, bits, cp.case_seed(M, K, C), dtype, backward=True,
                                     wide=wide)
    wref = (dY.double().t() @ X.double()).float()
    bref = dY.double().sum(0).float()
    Xd, _ = p16.nan_padded16(X, ldx_pad, DEV)
    Gd, _ = cp.nan_padded(dY, ldd_pad, DEV)
    assert _bwd_name(Xd, C) == kernel
    dW, db = linear_backward(Xd, Gd)
    assert torch.equal(dW.cpu(), wref)
    assert torch.equal(db.cpu(), bref)
    dW2, none = linear_backward(Xd, Gd, want_bias=False)
    assert none is None and torch.equal(dW2, dW)


# ---- 3. single-term probes ---------------------------------------------------------

@DT
@pytest.mark.parametrize("K,C", cp.SINGLE_TERM_SHAPES)
def test_forward_single_term(dtype, K, C):
    """Y[m, c] = float(x[m]) * W[c, m mod K], one product of a full-mantissa
    16-bit x and a full-mantissa fp32 w (M = 2 K + 1, no bias): within 2^-23
    for bf16 X (nothing dropped), 2^-22 for fp16 X; expected zeros exactly 0.
    Observed maxima, units of 2^-24: DESIGN 4.9."""
    M = 2 * K + 1
    X, W, ref = p16.single_term_forward_x16(M, K, C, cp.single_term_seed(M, K, C), dtype)
    Xd, _ = p16.nan_padded16(X, 2 - K % 2, DEV)
    assert _fwd_name(Xd)(C) == "linear_x16_kernel"
    Y = _linear_into_padded(Xd, W.to(DEV), None, C)
    worst, ok = cp.check_single_term(Y, ref, p16.BOUND[dtype])
    print(f"x16 single-term forward {dtype} K={K} C={C}: max rel err {worst:.3f} x 2^-24")
    assert ok, worst


@DT
@pytest.mark.parametrize("M,K,C,r0", cp.single_term_backward_cases())
def test_backward_single_term(dtype, M, K, C, r0):
    """dY non-zero on K consecutive rows from r0 (first, middle, last and
    partial): each dW[c, k] is one product dY[m, c] * float(x[m]) or exactly
    zero; with one element of dY per class db is that element bit for bit.
    Bounds as in the forward."""
    from sgc_amd.propagate import linear_backward
    X, dY, dYb, wref, wbref, bref = p16.single_term_backward_x16(
        M, K, C, r0, cp.single_term_seed(M, K, C) + r0, dtype)
    Xd, _ = p16.nan_padded16(X, 2 - K % 2, DEV)
    assert _bwd_name(Xd, C) == "xent_dw_cols_x16_kernel"
    dW, _ = linear_backward(Xd, dY.to(DEV))
    dWb, db = linear_backward(Xd, dYb.to(DEV))
    worst, ok = cp.check_single_term(dW.cpu(), wref, p16.BOUND[dtype])
    worst_b, ok_b = cp.check_single_term(dWb.cpu(), wbref, p16.BOUND[dtype])
    print(f"x16 single-term backward {dtype} M={M} K={K} C={C} r0={r0}: "
          f"max rel err {max(worst, worst_b):.3f} x 2^-24")
    assert ok and ok_b, (worst, worst_b)
    assert torch.equal(db.cpu(), bref)


# ---- 4. randn against fp64 torch of the upcast X -----------------------------------

@functools.lru_cache(maxsize=None)
def _randn_case(M, K, C, dtype):
    g = torch.Generator().manual_seed(M + K + C)
    X = torch.randn((M, K), generator=g).to(dtype)
    W = torch.randn((C, K), generator=g) / K ** 0.5
    b = torch.randn(C, generator=g)
    dY = torch.randn((M, C), generator=g) / M
    Y = F_.linear(X.double(), W.double(), b.double())
    dW = dY.double().t() @ X.double()
    return X, W, b, dY, Y, dW, dY.double().sum(0)


def _close(got, ref, what):
    tol = 1e-5 * float(ref.abs().max())
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=tol, msg=lambda m: f"{what}: {m}")


@DT
@pytest.mark.parametrize("M,K,C,pad", RANDN_SHAPES)
def test_randn_matches_fp64(dtype, M, K, C, pad):
    from sgc_amd.propagate import linear_backward
    X, W, b, dY, Yref, dWref, dbref = _randn_case(M, K, C, dtype)
    Xd, _ = p16.nan_padded16(X, pad, DEV)
    assert _fwd_name(Xd)(C) == "linear_x16_kernel"
    assert _bwd_name(Xd, C) == "xent_dw_cols_x16_kernel"
    _close(_linear_into_padded(Xd, W.to(DEV), b.to(DEV), C), Yref, "Y")
    dW, db = linear_backward(Xd, dY.to(DEV))
    _close(dW.cpu(), dWref, "dW")
    _close(db.cpu(), dbref, "db")


# ---- 5. non-finite features --------------------------------------------------------

@DT
def test_nonfinite_features(dtype):
    """+-inf and NaN at four (row, k) places of X: those rows of Y and those
    columns of dW are wholly non-finite (not necessarily torch's +-inf: the
    documented deviation), everything else stays within the randn tolerance
    and db is untouched."""
    from sgc_amd.propagate import linear_backward
    M, K, C, pad = RANDN_SHAPES[0]
    X0, W, b, dY, _, _, dbref = _randn_case(M, K, C, dtype)
    bad = {5: (100, float("inf")), 77: (3, float("-inf")), 500: (601, float("nan")),
           999: (0, float("inf"))}
    X = X0.clone()
    clean = X0.clone()
    for r, (k, v) in bad.items():
        X[r, k] = v
        clean[r, k] = 0
    rows = torch.tensor(sorted(bad))
    cols = torch.tensor(sorted(k for k, _ in bad.values()))
    good_r = torch.ones(M, dtype=torch.bool)
    good_r[rows] = False
    good_c = torch.ones(K, dtype=torch.bool)
    good_c[cols] = False
    Yref = F_.linear(clean.double(), W.double(), b.double())
    dWref = dY.double().t() @ clean.double()
    Xd, _ = p16.nan_padded16(X, pad, DEV)
    assert _fwd_name(Xd)(C) == "linear_x16_kernel"
    assert _bwd_name(Xd, C) == "xent_dw_cols_x16_kernel"
    Y = _linear_into_padded(Xd, W.to(DEV), b.to(DEV), C)
    assert not torch.isfinite(Y[rows]).any()
    _close(Y[good_r], Yref[good_r], "Y")
    dW, db = linear_backward(Xd, dY.to(DEV))
    dW = dW.cpu()
    assert not torch.isfinite(dW[:, cols]).any()
    _close(dW[:, good_c], dWref[:, good_c], "dW")
    _close(db.cpu(), dbref, "db")


# ---- 6. module level ---------------------------------------------------------------

@DT
@pytest.mark.parametrize("M,K,C", [(2000, 130, 41), (140, 1433, 7)])
def test_module_level(dtype, M, K, C):
    """F.cross_entropy(SGC(x16), y) with every seventh label ignore_index:
    the HIP loss, and loss / W.grad / b.grad against fp64 torch on x.double()
    (tolerances of test_logits_cross_entropy_matches_torch);
    sgc_cross_entropy(model, x16, y) is the same expression; one Adam step
    and one device L-BFGS step run and leave finite parameters."""
    from sgc_amd.models import SGC, sgc_cross_entropy
    from sgc_amd.optim import LBFGS
    torch.manual_seed(M + C)
    model = SGC(K, C).to(DEV)
    g = torch.Generator().manual_seed(K)
    x = torch.randn((M, K), generator=g).to(dtype)
    y = torch.randint(0, C, (M,), generator=g)
    y[3::7] = -100
    W64 = model.W.weight.detach().cpu().double().requires_grad_()
    b64 = model.W.bias.detach().cpu().double().requires_grad_()
    ref = F_.cross_entropy(F_.linear(x.double(), W64, b64), y)
    ref.backward()
    xd, yd = x.to(DEV), y.to(DEV)
    out = model(xd)
    assert out.dtype == torch.float32
    loss = F_.cross_entropy(out, yd)
    assert "LogitsCrossEntropy" in type(loss.grad_fn).__name__
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu().double(), ref.detach(), rtol=1e-5, atol=1e-6)
    gW, gb = model.W.weight.grad.clone(), model.W.bias.grad.clone()
    torch.testing.assert_close(gW.cpu().double(), W64.grad, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(gb.cpu().double(), b64.grad, rtol=1e-4, atol=1e-7)
    model.zero_grad()
    loss2 = sgc_cross_entropy(model, xd, yd)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach())
    assert torch.equal(model.W.weight.grad, gW) and torch.equal(model.W.bias.grad, gb)
    # a feature gradient, if asked for, has x's dtype
    xg = xd.clone().requires_grad_()
    F_.cross_entropy(model(xg), yd).backward()
    assert xg.grad.dtype == dtype and torch.isfinite(xg.grad.float()).all()

    def closure_of(opt):
        def closure():
            opt.zero_grad()
            value = F_.cross_entropy(model(xd), yd)
            value.backward()
            return value
        return closure

    adam = torch.optim.Adam(model.parameters(), lr=0.2)
    closure_of(adam)()
    adam.step()
    lb = LBFGS(model.parameters(), lr=1, max_iter=3)
    assert lb.device_path()
    lb.step(closure_of(lb))
    for p in model.parameters():
        assert torch.isfinite(p).all()


# ---- 7. pipeline -------------------------------------------------------------------

@DT
def test_pipeline_precompute_then_classify(tiny_cases, dtype):
    """sgc_precompute(X.to(T), adj, 2) returns dtype T and the model takes it
    as it is: logits within the randn tolerance of fp64 on X_K.double()."""
    from sgc_amd.models import SGC
    from sgc_amd.utils import sgc_precompute
    c = tiny_cases["hub1000_F130"]
    n = int(c["n"])
    idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64))
    adj = torch.sparse_coo_tensor(idx, torch.from_numpy(c["vals"]), (n, n)).to(DEV)
    X = torch.from_numpy(c["X"]).to(dtype).to(DEV)
    XK, _ = sgc_precompute(X, adj, 2)
    assert XK.dtype == dtype and XK.shape == X.shape
    torch.manual_seed(3)
    model = SGC(X.shape[1], 7).to(DEV)
    with torch.no_grad():
        got = model(XK).cpu()
    ref = F_.linear(XK.cpu().double(), model.W.weight.detach().cpu().double(),
                    model.W.bias.detach().cpu().double())
    _close(got, ref, "logits")


@pytest.mark.parametrize("name", ["bfloat16", "float16"])
def test_reddit_driver_feature_dtype(name):
    """drivers/reddit.py --synthetic 3000 --feature-dtype T through main(argv):
    a finite F1."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "drivers"))
    try:
        import reddit
    finally:
        sys.path.pop(0)
    f1, _, _ = reddit.main(["--synthetic", "3000", "--feature-dtype", name])
    assert np.isfinite(float(f1)) and 0.0 <= float(f1) <= 1.0


@pytest.mark.parametrize("name", ["bfloat16", "float16"])
def test_citation_driver_feature_dtype(name, tmp_path, monkeypatch):
    """drivers/citation.py --feature-dtype T on a synthetic Planetoid data set
    (Adam over 16-bit training rows): finite accuracies."""
    import json

    from planetoid_synth import write_planetoid
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "e2e_citation.json")) as f:
        golden = json.load(f)
    write_planetoid(str(tmp_path), **golden["dataset"])
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(here), "drivers"))
    import citation
    acc_val, acc_test = citation.main(["--dataset", "synth", "--epochs", "20", "--degree", "2",
                                       "--feature-dtype", name])
    assert np.isfinite(acc_val) and np.isfinite(acc_test) and 0.0 <= acc_test <= 1.0
