"""The classifier on 16-bit features without a GPU: the numpy model of the
x16 split scheme and its mutants on the single-term data, the integer
generators at the GPU tests' shapes, SGC on 16-bit CPU tensors, and the dtype
checks of the new C ABI (tests/classifier_probes_x16.py; the GPU side is
tests/test_gpu_classifier_x16.py)."""
import ctypes

import numpy as np
import pytest
import torch

import classifier_probes as cp
import classifier_probes_x16 as p16

F_ = torch.nn.functional
DT = pytest.mark.parametrize("dtype", p16.DTYPES, ids=["bf16", "fp16"])


# ---- the numpy model --------------------------------------------------------------

def _single_term_pairs(dtype, n=1 << 16, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = p16.full_mantissa_x16(g, (n,), dtype)
    w = cp.full_mantissa(g, (n,))
    return x, w


@DT
def test_full_mantissa_x16_properties(dtype):
    x, _ = _single_term_pairs(dtype)
    assert x.dtype == dtype and torch.isfinite(x.float()).all()
    nbits = 7 if dtype == torch.bfloat16 else 10
    raw = x.view(torch.int16).to(torch.int32) & 0xFFFF
    assert ((raw & 1) == 1).all()  # the lowest mantissa bit
    assert len(torch.unique(raw & ((1 << nbits) - 1))) == 1 << (nbits - 1)  # every odd mantissa
    a = x.float().abs()
    lo, hi = (2.0 ** -20, 2.0 ** 20) if dtype == torch.bfloat16 else (2.0 ** -10, 2.0 ** 10)
    assert a.min() >= lo and a.max() < hi
    pieces = p16.x_pieces(x.float().numpy(), dtype)
    total = sum(p.astype(np.float64) for p in pieces.values())
    assert np.array_equal(total, x.double().numpy())  # the pieces are x exactly
    if dtype == torch.float16:
        assert (pieces["m"] != 0).all()


@DT
def test_model_within_bound_and_mutants_outside(dtype):
    """On single-term data the intact scheme stays within its bound (2^-23
    for bf16 X, 2^-22 for fp16 X) and every scheme that leaves one product
    out exceeds it on more than half the elements."""
    x, w = _single_term_pairs(dtype)
    xf, wf = x.float().numpy(), w.numpy()
    ref = xf.astype(np.float64) * wf.astype(np.float64)
    err = cp.rel_err(p16.x16_product_model(xf, wf, dtype), ref)
    print(f"{dtype}: intact max rel err {err.max() * 2 ** 24:.3f} x 2^-24")
    assert err.max() <= p16.BOUND[dtype]
    for drop in p16.MUTANTS[dtype]:
        e = cp.rel_err(p16.x16_product_model(xf, wf, dtype, drop=drop), ref)
        share = float((e > p16.BOUND[dtype]).mean())
        print(f"{dtype}: without {drop}: {share:.4f} of the elements over the bound")
        assert share > p16.MUTANT_SHARE, (drop, share)


@DT
def test_single_term_layouts(dtype):
    K, C = 33, 17
    M = 2 * K + 1
    X, W, ref = p16.single_term_forward_x16(M, K, C, 3, dtype)
    assert X.dtype == dtype and (X != 0).sum(1).eq(1).all()
    assert torch.equal(F_.linear(X.double(), W.double()), ref)
    X, dY, dYb, wref, wbref, bref = p16.single_term_backward_x16(6145, K, C, 3001, 4, dtype)
    assert torch.equal(dY.double().t() @ X.double(), wref)
    assert torch.equal(dYb.double().t() @ X.double(), wbref)
    assert torch.equal(dYb.sum(0), bref) and (wref != 0).any()


# ---- integer operands at the GPU tests' shapes ------------------------------------

@DT
def test_integer_cases_are_exact_in_dtype(dtype):
    """Every integer case the GPU tests hand out is exactly representable in
    its dtype (the helper asserts it) and below 2^24 in every partial sum."""
    seen_m = False
    for (M, K, C, _pad, *modes, _k) in p16.FORWARD_CASES:
        if M > 5000:
            continue  # (the generator is the same; the GPU test builds these)
        bits, wide = p16.mode_of(modes, dtype)
        X, W, b = p16.integer_operands_x16(M, K, C, bits, cp.case_seed(M, K, C), dtype, wide=wide)
        assert X.dtype == dtype and W.dtype == torch.float32
        if dtype == torch.float16 and wide == "x" and bits == 10:
            seen_m = seen_m or bool((p16.x_pieces(X.float().numpy(), dtype)["m"] != 0).any())
    for (M, K, C, _px, _pd, *modes, _k) in p16.BACKWARD_CASES:
        if M > 5000:
            continue
        bits, wide = p16.mode_of(modes, dtype)
        X, dY = p16.integer_operands_x16(M, K, C, bits, cp.case_seed(M, K, C), dtype,
                                         backward=True, wide=wide)
        assert X.dtype == dtype and dY.dtype == torch.float32
    assert seen_m == (dtype == torch.float16)  # fp16's wide X has an m piece
    if dtype == torch.bfloat16:
        with pytest.raises(AssertionError):  # 10-bit integers are not bf16 values
            p16.integer_operands_x16(33, 33, 17, 10, 1, dtype, wide="x")


# ---- SGC on 16-bit CPU tensors ----------------------------------------------------

@DT
@pytest.mark.parametrize("M,K,C", [(7, 5, 3), (140, 1433, 7)])
def test_sgc_cpu_x16(dtype, M, K, C):
    """SGC(K, C)(x16) on CPU tensors is F.linear(x.float(), W, b) bit for bit,
    backward gives the gradients of that expression, and a feature gradient
    has x's dtype."""
    from sgc_amd.models import SGC, sgc_cross_entropy
    torch.manual_seed(M + K + C)
    m = SGC(K, C)
    x = torch.randn(M, K).to(dtype)
    y = torch.randint(0, C, (M,))
    out = m(x)
    assert out.dtype == torch.float32
    assert torch.equal(out, F_.linear(x.float(), m.W.weight, m.W.bias))
    xg = x.clone().requires_grad_()
    loss = F_.cross_entropy(m(xg), y)
    loss.backward()
    W2 = m.W.weight.detach().clone().requires_grad_()
    b2 = m.W.bias.detach().clone().requires_grad_()
    x2 = x.clone().requires_grad_()
    ref = F_.cross_entropy(F_.linear(x2.float(), W2, b2), y)
    ref.backward()
    assert torch.equal(loss, ref)
    assert torch.equal(m.W.weight.grad, W2.grad) and torch.equal(m.W.bias.grad, b2.grad)
    assert xg.grad.dtype == dtype and torch.equal(xg.grad, x2.grad)
    m.zero_grad()
    fused = sgc_cross_entropy(m, x, y)  # the unfused expression on the CPU
    assert torch.equal(fused, ref.detach())


# ---- the C ABI's dtype checks (no device call) ------------------------------------

def _lib():
    from sgc_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("bad", [0, 7])
def test_abi_rejects_other_dtypes_before_any_pointer(bad):
    lib = _lib()
    rc = lib.sgc_linear_x16(None, bad, 4, None, None, None, 4, 1, 3, 2, None)
    assert rc != 0
    msg = lib.sgc_last_error().decode()
    assert "x_dtype" in msg and str(bad) in msg, msg
    rc = lib.sgc_linear_backward_x16(None, bad, 4, None, 2, 1, 3, 2, None, None, None, 0, None)
    assert rc != 0
    msg = lib.sgc_last_error().decode()
    assert "x_dtype" in msg and str(bad) in msg, msg
    for name in (lib.sgc_linear_x16_kernel_name, lib.sgc_linear_backward_x16_kernel_name):
        assert name(16, 4, 4, 2, ctypes.c_void_p(4096), bad) == b"none"


def test_abi_names():
    lib = _lib()
    p = ctypes.c_void_p(4096)
    for dt, word in ((1, b"bf16"), (2, b"fp16")):
        fwd, bwd = lib.sgc_linear_x16_kernel_name, lib.sgc_linear_backward_x16_kernel_name
        assert fwd(0, 602, 602, 41, p, dt) == b"none" and bwd(0, 602, 602, 41, p, dt) == b"none"
        assert fwd(1, 602, 602, 41, p, dt).startswith(b"linear_x16_kernel") and word in fwd(
            1, 602, 602, 41, p, dt)
        assert bwd(1, 602, 602, 41, p, dt).startswith(b"xent_dw_cols_x16_kernel")
        assert fwd(100, 602, 602, 42, p, dt) != b"none"   # 162.3 KB of image: fits 160 KiB
        assert fwd(100, 602, 602, 43, p, dt) == b"none"   # a class block past LDS
        assert fwd(100, 602, 602, 49, p, dt) == b"none"
        assert bwd(100, 602, 602, 48, p, dt) != b"none" and bwd(100, 602, 602, 49, p, dt) == b"none"
        for f in (fwd, bwd):
            assert f(100, 31, 31, 16, p, dt) == b"none"                      # odd pitch
            assert f(100, 31, 32, 16, ctypes.c_void_p(4098), dt) == b"none"  # 2-B-aligned base
            assert f(100, 31, 32, 16, ctypes.c_void_p(4100), dt) != b"none"  # 4-B is enough
            assert f(1 << 20, 602, 1024, 41, p, dt) == b"none"               # M ldx 2 = 2^31
            assert f((1 << 20) - 1, 602, 1024, 41, p, dt) != b"none"
    assert lib.sgc_linear_backward_x16_workspace(0, 602, 41) == 0
    assert lib.sgc_linear_backward_x16_workspace(152410, 602, 41) >= 48 * 48 * 602 * 4


# ---- the citation driver's own flag (CPU mode) ------------------------------------

@pytest.mark.parametrize("name", ["bfloat16", "float16"])
def test_citation_driver_feature_dtype_cpu(name, tmp_path, monkeypatch):
    """drivers/citation.py --no-cuda --feature-dtype T on a synthetic Planetoid
    data set: the features are cast once, X_K and the training / evaluation
    rows stay in T, and the run ends with finite accuracies."""
    import json
    import os
    import sys

    from planetoid_synth import write_planetoid
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "e2e_citation.json")) as f:
        golden = json.load(f)
    write_planetoid(str(tmp_path), **golden["dataset"])
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(here), "drivers"))
    import citation
    seen = []
    real = citation.train_regression

    def spy(model, train_features, *rest):
        seen.append(train_features.dtype)
        return real(model, train_features, *rest)

    monkeypatch.setattr(citation, "train_regression", spy)
    acc_val, acc_test = citation.main(["--dataset", "synth", "--no-cuda", "--epochs", "20",
                                       "--degree", "2", "--feature-dtype", name])
    assert seen == [getattr(torch, name)]
    assert np.isfinite(acc_val) and np.isfinite(acc_test) and 0.0 <= acc_test <= 1.0
