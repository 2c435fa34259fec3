"""Device-resident evaluation on the GPU: sgc_linear_eval_f32 / _x16 at the raw
ABI, and propagate.linear_eval / SGC.predict / SGC.evaluate above them.

Exact problems (tests/eval_cases.py): integer operands make every logit exact
in fp32 in any summation order and in every bf16 split, so the predictions
must equal the first-maximum argmax of the int64 logits, the confusion matrix
its bincount and the counts exactly; the loss lies within rtol 1e-5 of fp64
(the bar sgc_cross_entropy_f32 states).

Random problems: X = standard_normal, W and b = 0.1 standard_normal rounded to
the operand types; the reference is the fp64 logits of the rounded operands
and tol = 1e-5 max |Z_ref| (the classifier's bar).  A row
is decided when its fp64 top-two gap exceeds 8 tol (two logits off by tol each
make 2 tol; the factor 4 keeps the test off the bound): decided rows must match
the fp64 argmax, an undecided row must get a class within 8 tol of the maximum,
and at most 0.5 % of a case's rows may be undecided.  Undecided rows of the
reference alone, computed on the CPU, seeds 0-4, per shape in RANDOM_SHAPES'
order:
    fp32  (6, 2, 2, 0, 2)  (6, 3, 5, 1, 3)  (4, 6, 5, 1, 3)  (4, 1, 2, 1, 0)  (6, 2, 6, 0, 3)
    bf16  (0, 2, 4, 2, 2)  (4, 4, 2, 0, 2)  (3, 0, 5, 0, 0)  (7, 1, 4, 2, 2)  (7, 1, 5, 1, 3)
    fp16  (5, 3, 3, 0, 1)  (7, 4, 4, 0, 3)  (1, 5, 5, 1, 3)  (3, 2, 4, 0, 0)  (5, 3, 9, 0, 2)
(one tuple per seed; at most 9 of 4149 rows, 0.22 %, and 2 of 1000).

Every output buffer is five elements longer than needed and pre-filled; the
slack must keep its fill (the ingest suite's convention).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import eval_cases as ec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "drivers"))
DEV = "cuda:0"
FILL = -7777
LOSS_FILL = 123.5
SGC_EINVAL, SGC_ENOMEM = 1, 4
OUTPUTS = ("pred", "confusion", "counts", "loss")
DTYPE_IDS = [ec.IDS[d] for d in ec.DTYPES]


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import _lib
    return _lib.load()


def _ptr(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def run_abi(lib, X, W, b, y, want=OUTPUTS, ws_short=0):
    """One raw call on the view X (device), W, b, y (device or None).  Returns
    (rc, {name: tensor without its slack}); asserts the slack kept its fill."""
    from sgc_amd import _lib
    M, K = X.shape
    C = W.shape[0]
    size = {"pred": M, "confusion": C * C, "counts": 2, "loss": 1}
    bufs = {}
    for name in OUTPUTS:
        if name in want:
            if name == "loss":
                bufs[name] = torch.full((size[name] + 5,), LOSS_FILL, dtype=torch.float32, device=DEV)
            else:
                bufs[name] = torch.full((size[name] + 5,), FILL, dtype=torch.int64, device=DEV)
    args_out = [_ptr(bufs.get(n)) for n in OUTPUTS]
    stream = _lib.stream_handle(X.device)
    if X.dtype == torch.float32:
        ws_bytes = lib.sgc_linear_eval_workspace(M, K, C)
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=DEV)
        rc = lib.sgc_linear_eval_f32(_ptr(X), X.stride(0), _ptr(W), _ptr(b), _ptr(y), M, K, C,
                                     *args_out, _ptr(ws), ws_bytes - ws_short, stream)
    else:
        ws_bytes = lib.sgc_linear_eval_x16_workspace(M, K, C)
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=DEV)
        rc = lib.sgc_linear_eval_x16(_ptr(X), ec.SGC_DTYPE[X.dtype], X.stride(0), _ptr(W), _ptr(b),
                                     _ptr(y), M, K, C, *args_out, _ptr(ws), ws_bytes - ws_short,
                                     stream)
    torch.cuda.synchronize()
    out = {}
    for name, t in bufs.items():
        fill = LOSS_FILL if name == "loss" else FILL
        assert bool((t[size[name]:] == fill).all()), f"{name}: the slack was written"
        out[name] = t[:size[name]].cpu()
    return rc, out


def kernel_name(lib, X, C):
    M, K = X.shape
    if X.dtype == torch.float32:
        return lib.sgc_linear_eval_kernel_name(M, K, X.stride(0), C, _ptr(X))
    return lib.sgc_linear_eval_x16_kernel_name(M, K, X.stride(0), C, _ptr(X), ec.SGC_DTYPE[X.dtype])


def check_exact(lib, X, W, b, layout, seed):
    """All four outputs of one exact problem against the int64 logits."""
    M, C = X.shape[0], W.shape[0]
    Z = ec.int_logits(X.float(), W, b)
    y = ec.labels_for(M, C, seed)
    Xd = ec.laid_out(X, layout, DEV)
    assert torch.equal(Xd.cpu(), X)
    assert kernel_name(lib, Xd, C) != b"none"
    rc, out = run_abi(lib, Xd, W.to(DEV), b.to(DEV), y.to(DEV))
    assert rc == 0, lib.sgc_last_error()
    pred_ref = Z.argmax(1)  # numpy: the first maximum
    got = out["pred"].numpy()
    assert np.array_equal(got, pred_ref), np.nonzero(got != pred_ref)[0][:10]
    cm, counts = ec.count_model(y.numpy(), pred_ref, C)
    assert np.array_equal(out["confusion"].numpy().reshape(C, C), cm)
    assert out["counts"].tolist() == counts.tolist()
    ref = ec.loss_fp64(Z, y.numpy())
    loss = float(out["loss"][0])
    print(f"loss {loss!r} fp64 {ref!r}")
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)


def _exact_params():
    for dtype in ec.DTYPES:
        shapes = ec.EXACT_SHAPES + (ec.EXACT_SHAPES_FP32 if dtype == torch.float32 else [])
        for (M, K, C, layouts) in shapes:
            for layout in layouts:
                yield pytest.param(dtype, M, K, C, layout,
                                   id=f"{ec.IDS[dtype]}-{M}x{K}x{C}-{layout}")


@pytest.mark.parametrize("dtype,M,K,C,layout", list(_exact_params()))
def test_exact_problems(lib, dtype, M, K, C, layout):
    X, W, b = ec.exact_operands(M, K, C, dtype, seed=1000 * M + C)
    check_exact(lib, X, W, b, layout, seed=M + K)


def _tie_params():
    for dtype in ec.DTYPES:
        shapes = [(37, 66, 41), (17, 130, 48), (4149, 66, 17), (15, 64, 2), (1, 64, 1)]
        if dtype == torch.float32:
            shapes.append((37, 66, 64))
        for (M, K, C) in shapes:
            yield pytest.param(dtype, M, K, C, id=f"{ec.IDS[dtype]}-{M}x{K}x{C}")


@pytest.mark.parametrize("dtype,M,K,C", list(_tie_params()))
def test_planted_ties_take_the_smallest_class(lib, dtype, M, K, C):
    for pair in ec.tie_pairs(C):
        X, W, b = ec.tie_operands(M, K, C, dtype, pair, seed=7 * M + C)
        check_exact(lib, X, W, b, "c", seed=M)
        if pair == "all":  # every class ties: class 0 wins every row
            rc, out = run_abi(lib, X.to(DEV), W.to(DEV), b.to(DEV), None, want=("pred",))
            assert rc == 0 and not out["pred"].any()


def _random_params():
    for dtype in ec.DTYPES:
        for (M, K, C) in ec.RANDOM_SHAPES:
            yield pytest.param(dtype, M, K, C, id=f"{ec.IDS[dtype]}-{M}x{K}x{C}")


@pytest.mark.parametrize("dtype,M,K,C", list(_random_params()))
def test_random_problems_decided_rows(lib, dtype, M, K, C):
    for seed in ec.RANDOM_SEEDS:
        X, W, b, Z, tol = ec.random_problem(M, K, C, seed, dtype)
        y = ec.labels_for(M, C, seed)
        rc, out = run_abi(lib, X.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV))
        assert rc == 0, lib.sgc_last_error()
        pred = out["pred"].numpy()
        assert pred.min() >= 0 and pred.max() < C
        undecided, wrong, far = ec.check_random(pred, Z, tol)
        print(f"seed {seed}: undecided {undecided} of {M}, decided wrong {wrong}, undecided far {far}")
        assert undecided <= ec.UNDECIDED_SHARE * M
        assert wrong == 0 and far == 0
        cm, counts = ec.count_model(y.numpy(), pred, C)
        assert np.array_equal(out["confusion"].numpy().reshape(C, C), cm)
        assert out["counts"].tolist() == counts.tolist()
        ref = ec.loss_fp64(Z, y.numpy())
        assert abs(float(out["loss"][0]) - ref) <= 1e-5 * abs(ref), (float(out["loss"][0]), ref)


# (M, K, C, pad), ldx = K + pad: the smallest shapes at which the x16 stream takes another path
ONE_STREAM_SHAPES = [
    (1, 8, 1, 0),       # one half chunk, NT = 1
    (16, 9, 17, 1),     # the second half chunk with one live k (the kernels need an even pitch:
                        # K = 9 is covered from ldx = 10 on, its tightest layout)
    (37, 66, 41, 0),    # a ragged double chunk whose second half is dropped, a partial row
    (37, 66, 41, 2),    # tile, a partial last class tile
    (33, 130, 64, 0),   # NT = 4, every class tile full
    (4149, 64, 17, 0),  # 260 tiles: a workgroup of a 256-CU part takes a second tile
]


@pytest.mark.parametrize("M,K,C,pad", ONE_STREAM_SHAPES,
                         ids=[f"{M}x{K}x{C}-ldx{K + pad}" for (M, K, C, pad) in ONE_STREAM_SHAPES])
@pytest.mark.parametrize("dtype", ec.DTYPES[1:], ids=DTYPE_IDS[1:])
def test_x16_predictions_are_the_argmax_of_linear_x16_logits(lib, dtype, M, K, C, pad):
    """The forwards are one stream: sgc_linear_eval_x16 and sgc_linear_x16 form
    the same accH + accL + bias bits, so on random operands every row's
    prediction is the argmax of the other entry's logits -- no decided-rows
    filter, no tolerance.  The padding of a pitch above K holds NaN."""
    from sgc_amd import _lib
    g = torch.Generator().manual_seed(1000 * M + 10 * K + C)
    X = torch.randn((M, K), generator=g).to(dtype)
    W, b = torch.randn((C, K), generator=g), torch.randn((C,), generator=g)
    Xd, Wd, bd = ec.cp.nan_padded(X, pad, DEV)[0], W.to(DEV), b.to(DEV)
    assert torch.equal(Xd.cpu(), X) and Xd.stride(0) == K + pad
    Y = torch.full((M, C), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.sgc_linear_x16(_ptr(Xd), ec.SGC_DTYPE[dtype], Xd.stride(0), _ptr(Wd), _ptr(bd), _ptr(Y),
                            Y.stride(0), M, K, C, _lib.stream_handle(Xd.device))
    assert rc == 0, lib.sgc_last_error()
    rc, out = run_abi(lib, Xd, Wd, bd, None, want=("pred",))
    assert rc == 0, lib.sgc_last_error()
    want = Y.cpu().max(1)[1]
    assert torch.equal(out["pred"], want), torch.nonzero(out["pred"] != want)[:10].tolist()


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=DTYPE_IDS)
def test_special_values_through_the_bias(lib, dtype):
    """The bias is added exactly after the MFMAs: a NaN class wins every row
    (the first of two), +inf wins, -inf everywhere but one class leaves it."""
    M, K, C = 37, 66, 41
    X, W, b0 = ec.tie_operands(M, K, C, dtype, (0, 1), seed=11)
    y = ec.labels_for(M, C, 3)

    def bias(**at):
        b = b0.clone()
        for c, v in at.items():
            b[int(c[1:])] = v
        return b

    everywhere = torch.full((C,), -INF)
    everywhere[3] = 2.0
    for b, winner in ((bias(c5=NAN), 5), (bias(c20=NAN, c7=NAN), 7), (bias(c40=INF), 40),
                      (everywhere, 3)):
        rc, out = run_abi(lib, X.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV))
        assert rc == 0, lib.sgc_last_error()
        assert (out["pred"] == winner).all(), (winner, out["pred"])
        cm, counts = ec.count_model(y.numpy(), np.full(M, winner), C)
        assert np.array_equal(out["confusion"].numpy().reshape(C, C), cm)
        assert out["counts"].tolist() == counts.tolist()


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=DTYPE_IDS)
def test_argument_forms(lib, dtype):
    M, K, C = 129, 66, 17
    X, W, b = ec.exact_operands(M, K, C, dtype, seed=5)
    Z = ec.int_logits(X.float(), W, b)
    y = ec.labels_for(M, C, 8)
    pred_ref = Z.argmax(1)
    cm, counts = ec.count_model(y.numpy(), pred_ref, C)
    ref = {"pred": pred_ref.tolist(), "confusion": cm.reshape(-1).tolist(), "counts": counts.tolist()}
    Xd, Wd, bd, yd = X.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV)

    def check(out):
        for name, t in out.items():
            if name == "loss":
                want = ec.loss_fp64(Z, y.numpy())
                assert abs(float(t[0]) - want) <= 1e-5 * abs(want)
            else:
                assert t.tolist() == ref[name], name

    # labels = NULL: predictions only
    rc, out = run_abi(lib, Xd, Wd, bd, None, want=("pred",))
    assert rc == 0 and sorted(out) == ["pred"]
    check(out)
    # ... and the other outputs are then refused
    for name in ("confusion", "counts", "loss"):
        rc, _ = run_abi(lib, Xd, Wd, bd, None, want=("pred", name))
        assert rc == SGC_EINVAL and b"labels" in lib.sgc_last_error()
    # b = NULL
    rc, out = run_abi(lib, Xd, Wd, None, yd, want=("pred",))
    assert rc == 0 and out["pred"].tolist() == ec.int_logits(X.float(), W, 0 * b).argmax(1).tolist()
    # each output NULL in turn, and each alone
    for name in OUTPUTS:
        rc, out = run_abi(lib, Xd, Wd, bd, yd, want=tuple(n for n in OUTPUTS if n != name))
        assert rc == 0 and name not in out, lib.sgc_last_error()
        check(out)
        rc, out = run_abi(lib, Xd, Wd, bd, yd, want=(name,))
        assert rc == 0 and sorted(out) == [name], lib.sgc_last_error()
        check(out)
    rc, _ = run_abi(lib, Xd, Wd, bd, yd, want=())
    assert rc == SGC_EINVAL


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=DTYPE_IDS)
def test_out_of_range_label_is_left_out(lib, dtype):
    M, K, C = 37, 66, 41
    X, W, b = ec.exact_operands(M, K, C, dtype, seed=6)
    y = ec.labels_for(M, C, 9)
    y[4], y[36], y[17] = C, -1, 2 ** 40  # (the last row of a ragged tile among them)
    pred_ref = ec.int_logits(X.float(), W, b).argmax(1)
    rc, out = run_abi(lib, X.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV))
    assert rc == 0, lib.sgc_last_error()
    cm, counts = ec.count_model(y.numpy(), pred_ref, C)
    assert counts[0] == M - 3
    assert out["pred"].tolist() == pred_ref.tolist()
    assert np.array_equal(out["confusion"].numpy().reshape(C, C), cm)
    assert out["counts"].tolist() == counts.tolist()
    assert torch.isnan(out["loss"][0])


def test_error_returns_and_names(lib):
    K = 66
    X32 = torch.zeros((8, K + 2), dtype=torch.float32, device=DEV)
    X16 = torch.zeros((8, K + 2), dtype=torch.bfloat16, device=DEV)
    W = torch.zeros((64, K), dtype=torch.float32, device=DEV)
    pred = torch.full((16,), FILL, dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)

    def f32(M, K_, ldx, C, ws_bytes=1 << 20, X=X32):
        return lib.sgc_linear_eval_f32(_ptr(X), ldx, _ptr(W), None, None, M, K_, C, _ptr(pred), None,
                                       None, None, _ptr(ws), ws_bytes, None)

    def x16(M, K_, ldx, C, dt=1, ws_bytes=1 << 20, X=X16):
        return lib.sgc_linear_eval_x16(_ptr(X), dt, ldx, _ptr(W), None, None, M, K_, C, _ptr(pred),
                                       None, None, None, _ptr(ws), ws_bytes, None)

    def n32(M, K_, ldx, C, X=X32):
        return lib.sgc_linear_eval_kernel_name(M, K_, ldx, C, _ptr(X))

    def n16(M, K_, ldx, C, dt=1, X=X16):
        return lib.sgc_linear_eval_x16_kernel_name(M, K_, ldx, C, _ptr(X), dt)

    assert n32(8, K, K + 2, 17) != b"none" and n16(8, K, K + 2, 17) != b"none"
    assert n16(8, K, K + 2, 17, dt=2) != b"none"
    bad = [
        (8, K, K + 2, 0), (8, K, K + 2, 65),            # C = 0, C = 65
        (8, K, K - 2, 17),                               # ldx < K
        (1 << 20, K, 1 << 10, 17),                       # M * ldx * size >= 2^31
        (0, K, K + 2, 17),
    ]
    for (M, K_, ldx, C) in bad:
        for call, name in ((f32, n32), (x16, n16)):
            assert call(M, K_, ldx, C) == SGC_EINVAL, (M, K_, ldx, C)
            assert lib.sgc_last_error()
            assert name(M, K_, ldx, C) == b"none", (M, K_, ldx, C)
    assert (1 << 19) * (1 << 10) * 4 >= 2 ** 31 > (1 << 19) * (1 << 10) * 2  # the two sizes differ
    assert n32(1 << 19, K, 1 << 10, 17) == b"none" and n16(1 << 19, K, 1 << 10, 17) != b"none"
    # x16: odd pitch, unknown dtype, a 2-B-aligned base
    assert x16(8, K, K + 1, 17) == SGC_EINVAL and n16(8, K, K + 1, 17) == b"none"
    for dt in (0, 3, -1):
        assert x16(8, K, K + 2, 17, dt=dt) == SGC_EINVAL and n16(8, K, K + 2, 17, dt=dt) == b"none"
        assert b"x_dtype" in lib.sgc_last_error()
    assert lib.sgc_linear_eval_x16_kernel_name(8, K, K + 2, 17, _ptr(X16, 2), 1) == b"none"
    assert lib.sgc_linear_eval_kernel_name(8, K, K + 2, 17, _ptr(X32, 2)) == b"none"
    # K = 602: W's image fits LDS up to 42 classes
    assert n16(4096, 602, 602, 42) != b"none" and n16(4096, 602, 602, 43) == b"none"
    assert lib.sgc_linear_eval_x16_workspace(4096, 602, 43) == 0
    assert lib.sgc_linear_eval_workspace(8, K, 65) == 0
    # the workspace one byte short
    need32 = lib.sgc_linear_eval_workspace(8, K, 17)
    need16 = lib.sgc_linear_eval_x16_workspace(8, K, 17)
    assert 0 < need32 <= 1 << 20 and 0 < need16 <= 1 << 20
    assert f32(8, K, K + 2, 17, ws_bytes=need32 - 1) == SGC_ENOMEM
    assert x16(8, K, K + 2, 17, ws_bytes=need16 - 1) == SGC_ENOMEM
    assert f32(8, K, K + 2, 17, ws_bytes=need32) == 0 and x16(8, K, K + 2, 17, ws_bytes=need16) == 0
    torch.cuda.synchronize()
    assert not pred[:8].any() and bool((pred[8:] == FILL).all())  # nothing before was written


def test_reproducible_run_to_run(lib):
    """bf16, dynamic tiles: the same loss bits and the same integers twice."""
    M, K, C = 4149, 66, 17
    X, W, b, _, _ = ec.random_problem(M, K, C, 0, torch.bfloat16)
    y = ec.labels_for(M, C, 0)
    Xd, Wd, bd, yd = X.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV)
    runs = [run_abi(lib, Xd, Wd, bd, yd)[1] for _ in range(2)]
    for name in ("pred", "confusion", "counts"):
        assert torch.equal(runs[0][name], runs[1][name])
    assert torch.equal(runs[0]["loss"].view(torch.int32), runs[1]["loss"].view(torch.int32))


# ---- the Python surface -------------------------------------------------------------

def _model(W, b):
    from sgc_amd.models import SGC
    model = SGC(W.shape[1], W.shape[0])
    with torch.no_grad():
        model.W.weight.copy_(W)
        model.W.bias.copy_(b)
    return model.to(DEV)


def check_surface(model, x, y):
    from sgc_amd.metrics import accuracy, f1
    with torch.no_grad():
        out = model(x)
    ev = model.evaluate(x, y)
    assert ev.confusion.device == x.device and ev.loss.device == x.device
    assert torch.equal(ev.accuracy(), accuracy(out, y))
    micro, macro = ev.f1()
    ref_micro, ref_macro = f1(out, y)
    assert abs(micro - ref_micro) <= 1e-12 and abs(macro - ref_macro) <= 1e-12
    assert torch.equal(model.predict(x), out.max(1)[1])
    assert int(ev.count) == len(y)
    ref_loss = float(torch.nn.functional.cross_entropy(out.double().as_subclass(torch.Tensor), y))
    assert abs(float(ev.loss) - ref_loss) <= 1e-5 * abs(ref_loss)


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=DTYPE_IDS)
def test_evaluate_and_predict_equal_the_literal_expressions(lib, dtype):
    M, K, C = 4149, 66, 17
    X, W, b = ec.exact_operands(M, K, C, dtype, seed=21)
    x, y = X.to(DEV), ec.labels_for(M, C, 4).to(DEV)
    assert kernel_name(lib, x, C) != b"none"
    check_surface(_model(W, b), x, y)


def test_fallbacks_outside_coverage(lib):
    # 70 classes: the logits from `linear`, then torch ops
    for dtype in (torch.float32, torch.bfloat16):
        X, W, b = ec.exact_operands(129, 66, 70, dtype, seed=22)
        x, y = X.to(DEV), ec.labels_for(129, 70, 5).to(DEV)
        assert kernel_name(lib, x, 70) == b"none"
        check_surface(_model(W, b), x, y)
    # a contiguous 37 x 67 bf16 tensor: odd pitch, one even-pitch copy, then the kernel
    X, W, b = ec.exact_operands(37, 67, 41, torch.bfloat16, seed=23)
    x, y = X.to(DEV), ec.labels_for(37, 41, 6).to(DEV)
    assert x.stride(0) == 67 and kernel_name(lib, x, 41) == b"none"
    check_surface(_model(W, b), x, y)
    # CPU tensors
    model = _model(W, b).cpu()
    ev = model.evaluate(X, y.cpu())
    assert ev.confusion.device.type == "cpu"
    assert torch.equal(model.predict(X), torch.from_numpy(ec.int_logits(X.float(), W, b).argmax(1)))


def test_evaluate_checks_labels_once_per_tensor_and_version():
    """The label check (one host synchronisation) belongs to the labels tensor
    object and its version: a second call on the same tensor does not look at
    the labels again, an in-place write does."""
    from sgc_amd import models
    C = 7
    X, W, b = ec.exact_operands(37, 66, C, torch.float32, seed=24)
    model, x = _model(W, b), X.to(DEV)
    y = ec.labels_for(37, C, 7).to(DEV)
    ev = model.evaluate(x, y)
    ref, state = models._checked_labels[id(y)]
    assert ref() is y and state == (y._version, C, 0)
    # a write behind the version counter: the cached pass stands, so nothing raises, and the
    # kernels leave the row out (count 36, NaN loss) -- the check did not run again
    y.data[5] = C
    assert y._version == state[0]
    again = model.evaluate(x, y)
    assert int(ev.count) == 37 and int(again.count) == 36 and bool(torch.isnan(again.loss))
    y.data[5] = 0
    y[5] = C  # an in-place write: a new version, checked again
    assert y._version != state[0]
    with pytest.raises(IndexError):
        model.evaluate(x, y)
    # another tensor object with the same values is checked on its own
    with pytest.raises(IndexError):
        model.evaluate(x, y.clone())
    with pytest.raises(IndexError, match="Target -100"):  # torch's ignore_index is not skipped
        model.evaluate(x, torch.full_like(y, -100))


# ---- the drivers ----------------------------------------------------------------------

def _count_evaluate_calls(monkeypatch):
    """Wrap SGC.evaluate; returns the list its calls are appended to."""
    from sgc_amd.models import SGC
    calls = []
    inner = SGC.evaluate

    def counted(self, x, labels):
        calls.append(tuple(x.shape))
        return inner(self, x, labels)

    monkeypatch.setattr(SGC, "evaluate", counted)
    return calls


def test_citation_driver_device_eval_gives_the_same_accuracies(tmp_path, monkeypatch):
    """citation.py's parsers drop unknown flags, so equal accuracies alone would
    not tell a routed --device-eval from an ignored one: with the flag the
    validation and the test accuracy each come from one SGC.evaluate call,
    without it from none."""
    import citation
    from planetoid_synth import write_planetoid
    with open(os.path.join(HERE, "golden", "e2e_citation.json")) as f:
        golden = json.load(f)
    write_planetoid(str(tmp_path), **golden["dataset"])
    monkeypatch.chdir(tmp_path)
    calls = _count_evaluate_calls(monkeypatch)
    argv = [a for a in golden["reference_citation_py"]["args"] if a != "--no-cuda"]
    plain = citation.main(argv)
    assert calls == []
    device = citation.main(argv + ["--device-eval"])
    spec = golden["dataset"]
    assert len(calls) == 2 and calls[1][0] == spec.get("n_test", 300), calls  # val, then test rows
    assert plain == device, (plain, device)


def test_reddit_driver_device_eval_gives_the_same_f1(monkeypatch):
    import reddit
    calls = _count_evaluate_calls(monkeypatch)
    plain = reddit.main(["--synthetic", "4096"])[0]
    assert calls == []
    device = reddit.main(["--synthetic", "4096", "--device-eval"])[0]
    assert len(calls) == 1 and calls[0][1] == 602, calls
    assert abs(plain - device) <= 1e-12, (plain, device)
