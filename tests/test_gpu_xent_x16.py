"""sgc_linear_xent_x16 on the GPU: the fused training step on bf16 / fp16
features against fp64 torch on the exactly widened X (the tolerances of
test_gpu_parity.py::test_fused_xent_matches_torch), integer operands (loss to
1 ulp), the fp32 fused step on X.float() (ours <= 2 x fp32's error + FLOOR),
bitwise reproducibility (what per-wave loss partials would break), and
propagate.linear_xent's 16-bit path.

Shapes: the smallest at which each mechanism can break -- M around the 16-row
tile and past the launch's workgroup count (a workgroup then takes several
tiles), K around the 64-k double chunk and the half-chunk rule (K - 1) % 64 < 8,
C around the 16-class tile up to 48, ldx > K and a base that is 4-B but not
16-B aligned."""
import math

import pytest
import torch

from adam_ref import FLOOR, rel_err, xent_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = (torch.bfloat16, torch.float16)
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def past_workgroups():
    """An M with more 16-row tiles than the launch has workgroups (one per CU)."""
    return 16 * (n_cus() + 3) + 5


def problem(M, K, C, seed=1, ints=False):
    """tests/test_gpu_adam.py's problem(): sparse-ish citation-like features
    (or small integers), fp32 on the CPU."""
    gen = torch.Generator().manual_seed(seed + 31 * M + K)
    y = torch.randint(0, C, (M,), generator=gen)
    if ints:
        X = torch.randint(0, 3, (M, K), generator=gen).float()
        W = torch.randint(-1, 2, (C, K), generator=gen).float()
        b = torch.randint(-2, 3, (C,), generator=gen).float()
        return X, W, b, y
    cent = torch.randn(C, K, generator=gen) * 0.05
    X = (torch.rand(M, K, generator=gen) < 0.01).float() * 0.1 + cent[y].abs() * 0.2
    W = (torch.rand(C, K, generator=gen) * 2 - 1) / math.sqrt(K)
    b = (torch.rand(C, generator=gen) * 2 - 1) / math.sqrt(K)
    return X, W, b, y


def lay(X16, layout):
    """X16 on the device: contiguous, ldx = K + 6, or a base two elements past
    an aligned address (4-B aligned, not 16-B aligned)."""
    M, K = X16.shape
    if layout == "pad":
        buf = torch.full((M, K + 6), float("nan"), dtype=X16.dtype, device=DEV)
        out = buf[:, :K]
    elif layout == "offset":
        flat = torch.zeros(M * K + 2, dtype=X16.dtype, device=DEV)
        out = flat[2:].view(M, K)
        assert out.data_ptr() % 16 == 4
    else:
        return X16.to(DEV)
    out.copy_(X16)
    return out


def raw_step(X, W, b, y):
    """One sgc_linear_xent_x16 call on X as it lies in memory -> (loss, dW, db)."""
    from sgc_amd import _lib
    from sgc_amd.propagate import X16_DTYPES
    lib = _lib.load()
    M, K = X.shape
    C = W.shape[0]
    dt = X16_DTYPES[X.dtype]
    assert lib.sgc_linear_xent_x16_kernel_name(M, K, X.stride(0), C, _lib.ptr(X), dt) != b"none"
    ws_bytes = lib.sgc_linear_xent_x16_workspace(M, K, C)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    loss = torch.empty((), device=DEV)
    dW = torch.empty_like(W)
    db = None if b is None else torch.empty_like(b)
    _lib.check(lib.sgc_linear_xent_x16(_lib.ptr(X), dt, X.stride(0), _lib.ptr(W), _lib.ptr(b),
                                       _lib.ptr(y), M, K, C, _lib.ptr(loss), _lib.ptr(dW),
                                       _lib.ptr(db), _lib.ptr(ws), ws_bytes,
                                       _lib.stream_handle(DEV)), "linear_xent_x16")
    return loss, dW, db


def cases():
    big = ("big", 66, 7)
    out = [(M, 66, 17, "contiguous") for M in (1, 15, 16, 17, 129)]
    out += [(big[0], big[1], big[2], "contiguous")]
    out += [(37, K, 41, "contiguous") for K in (2, 62, 64, 66, 72, 130, 602)]
    out += [(129, 130, C, "contiguous") for C in (1, 16, 17, 41, 48)]
    out += [(129, 66, 17, lay_) for lay_ in ("pad", "offset")]
    out += [(37, 602, 41, lay_) for lay_ in ("pad", "offset")]
    out += [(1, 2, 1, "pad"), (17, 72, 48, "offset")]
    return out


def case_id(c):
    return "%sx%dx%d-%s" % c


_cache = {}


def setup(case, dtype, ints=False):
    """(device operands, fp64 reference (loss, dW, db)), computed once."""
    key = (case, dtype, ints)
    if key not in _cache:
        M, K, C, layout = case
        if M == "big":
            M = past_workgroups()
        X, W, b, y = problem(M, K, C, ints=ints)
        X16 = X.to(dtype)
        if ints:
            assert torch.equal(X16.float(), X)
        Xd, Wd, bd, yd = lay(X16, layout), W.to(DEV), b.to(DEV), y.to(DEV)
        ref = xent_grads(Xd.double(), Wd.double(), bd.double(), yd)
        _cache[key] = ((Xd, Wd, bd, yd), tuple(t.clone() for t in ref))
    return _cache[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_matches_fp64_torch_on_the_widened_features(case, dtype):
    (X, W, b, y), (rl, rW, rb) = setup(case, dtype)
    loss, dW, db = raw_step(X, W, b, y)
    torch.testing.assert_close(loss.double(), rl, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dW.double(), rW, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(db.double(), rb, rtol=1e-4, atol=1e-6)
    # no bias: db is not touched and the loss is the bias-free one
    loss0, dW0, _ = raw_step(X, W, None, y)
    r0 = xent_grads(X.double(), W.double(), None, y)
    torch.testing.assert_close(loss0.double(), r0[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dW0.double(), r0[1], rtol=1e-4, atol=1e-6)


INT_CASES = [(129, 66, 17, "contiguous"), (37, 602, 41, "pad"), ("big", 66, 7, "contiguous"),
             (60, 500, 3, "offset"), (17, 72, 48, "contiguous")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", INT_CASES, ids=case_id)
def test_integer_operands_loss_to_one_ulp(case, dtype):
    """Small-integer X, W and b give exact logits: the loss equals the fp64
    value to 1 ulp (a dropped or doubled chunk moves it by far more)."""
    (X, W, b, y), (rl, _, _) = setup(case, dtype, ints=True)
    loss, _, _ = raw_step(X, W, b, y)
    want = rl.float()
    ulp = float(torch.nextafter(want, want + 1) - want)
    print(f"integer probe {case} {IDS[dtype]}: loss {float(loss)!r} fp64 {float(rl)!r} ulp {ulp:.3e}")
    assert abs(float(loss) - float(rl)) <= ulp


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", [(129, 66, 17, "contiguous"), (37, 602, 41, "contiguous"),
                                  (129, 130, 48, "contiguous"), (3000, 602, 41, "contiguous")],
                         ids=case_id)
def test_no_worse_than_the_fp32_fused_step(case, dtype):
    """err(x16 vs fp64) <= 2 err(fp32 step on X.float() vs fp64) + FLOOR."""
    from sgc_amd.propagate import linear_xent
    (X, W, b, y), ref = setup(case, dtype)
    ours = raw_step(X, W, b, y)
    f32 = linear_xent(X.float(), W, b, y)
    for name, o, f, r in zip(("loss", "dW", "db"), ours, f32, ref):
        eo, ef = rel_err(o, r), rel_err(f, r)
        print(f"xent x16 {case} {IDS[dtype]}: {name}: e(x16)={eo:.3e} e(fp32 step)={ef:.3e}")
    for name, o, f, r in zip(("loss", "dW", "db"), ours, f32, ref):
        assert rel_err(o, r) <= 2 * rel_err(f, r) + FLOOR, name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", [(3000, 602, 41, "contiguous"), ("big", 66, 7, "contiguous")],
                         ids=case_id)
def test_five_runs_give_the_same_bits(case, dtype):
    (X, W, b, y), _ = setup(case, dtype)
    first = raw_step(X, W, b, y)
    for _ in range(4):
        again = raw_step(X, W, b, y)
        for a, c in zip(first, again):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_propagate_linear_xent(dtype):
    from sgc_amd import _lib
    from sgc_amd.propagate import X16_DTYPES, linear, linear_xent
    lib = _lib.load()
    # an odd pitch goes through the even-pitch copy and meets the same tolerance
    X, W, b, y = problem(70, 33, 3)
    X16 = X.to(dtype).to(DEV)
    W, b, y = W.to(DEV), b.to(DEV), y.to(DEV)
    assert lib.sgc_linear_xent_x16_kernel_name(70, 33, 33, 3, _lib.ptr(X16),
                                               X16_DTYPES[dtype]) == b"none"
    out = linear_xent(X16, W, b, y)
    assert len(out) == 3 and all(t.dtype == torch.float32 for t in out)
    rl, rW, rb = xent_grads(X16.double(), W.double(), b.double(), y)
    torch.testing.assert_close(out[0].double(), rl, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out[1].double(), rW, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(out[2].double(), rb, rtol=1e-4, atol=1e-6)
    # a covered layout runs the x16 step itself: the raw call's bits
    (Xc, Wc, bc, yc), _ = setup((129, 66, 17, "pad"), dtype)
    got = linear_xent(Xc, Wc, bc, yc, want_logits=True)
    raw = raw_step(Xc, Wc, bc, yc)
    assert all(torch.equal(a, c) for a, c in zip(got[:3], raw))
    assert torch.equal(got[3], linear(Xc, Wc, bc))
    # no bias
    assert linear_xent(Xc, Wc, None, yc)[2] is None
    bad = yc.clone()
    bad[3] = 17
    with pytest.raises(ValueError):
        linear_xent(Xc, Wc, bc, bad)
