"""sgc_linear_xent_x16 on the GPU where tests/test_gpu_xent_x16.py cannot see:
the logits of launch A (xent_fwd_x16_kernel has no logits output) and its
softmax away from |z| < 1.

* single-term step: each window row's logits are one product of full-mantissa
  operands and its dW column one term, so M * dW[:, k_m] / x_m reads launch
  A's G row by row: e(x16) <= 2 e(fp32 step) + FLOOR -- a bound every
  drop-one-product scheme exceeds eightfold (test_xent_x16_probes_cpu.py);
* softmax edges: offsets of 0, +-1000, +-30000 through the bias, rows that
  lead by 256 and 8192, flat rows, C = 1 .. 48, at test_fused_xent_softmax_
  edges's tolerances against fp64 cross-entropy of the exactly known fp32
  logits;
* the fused loops on an edge problem: the first loss of sgc_train_adam_x16 and
  of sgc_train_lbfgs_x16 has the raw step's bits;
* the top of the covered pitch range, M * ldx * 2 just under 2^31.

Operands, the model and the verdicts: tests/xent_x16_probes.py."""
import pytest
import torch

import classifier_probes as cp
import classifier_probes_x16 as p16
import xent_x16_probes as xp
from adam_ref import FLOOR, xent_grads
from test_gpu_xent_x16 import DEV, DTYPES, IDS, lay, past_workgroups, problem, raw_step

pytestmark = pytest.mark.gpu

F_ = torch.nn.functional
DT = pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. the single-term step ------------------------------------------------------

SINGLE = [case + ("contiguous",) for case in xp.SINGLE_TERM_CASES] + \
    [(37, 66, 41, 0, "pad"), (37, 66, 41, 0, "offset")]


def single_id(c):
    M, K, C, r0, layout = c
    return "%sx%dx%d-r0=%s-%s" % ("big" if M is None else M, K, C, "M-64" if r0 is None else r0,
                                  layout)


@DT
@pytest.mark.parametrize("case", SINGLE, ids=single_id)
def test_single_term_step_reads_launch_a_row_by_row(case, dtype):
    """e = max |M dW[:, k_m] / x_m - G64[m, :]| of the x16 step is at most twice
    that of the fp32 step on X.float() plus FLOOR; columns no window row owns
    are exactly zero; loss and db meet test_gpu_xent_x16.py's tolerances
    against fp64.  Measured e: DESIGN 4.12."""
    from sgc_amd.propagate import linear_xent
    M, K, C, r0, layout = case
    M = past_workgroups() if M is None else M
    r0 = M - 64 if r0 is None else r0
    p = xp.single_term_step(M, K, C, r0, xp.single_term_seed(M, K, C, r0), dtype)
    Xd = lay(p.X, layout)
    if layout == "pad":
        assert Xd.stride(0) == K + 6
    Wd, yd, zeros = p.W.to(DEV), p.y.to(DEV), torch.zeros(C, device=DEV)
    ours = raw_step(Xd, Wd, zeros, yd)
    f32 = linear_xent(p.X.float().to(DEV), Wd, zeros, yd)
    e32, _ = xp.single_term_error(p, f32[1])
    e, bad = xp.check_single_term(p, ours, e32)
    print(f"xent x16 single-term {single_id(case)} M={M} {IDS[dtype]}: e(x16)={e / FLOOR:.3f} "
          f"e(fp32 step)={e32 / FLOOR:.3f} FLOOR")
    assert bad == [], (bad, e / FLOOR, e32 / FLOOR)
    # without a bias: the same G, so the same dW bits
    assert same_bits(raw_step(Xd, Wd, None, yd)[1], ours[1])


# ---- 2. softmax edges --------------------------------------------------------------

EDGE_MS = (7, 1000, "big")


@DT
@pytest.mark.parametrize("C", [1, 3, 17, 41, 48])
@pytest.mark.parametrize("M", EDGE_MS)
def test_softmax_edges(M, C, dtype):
    """Offsets 0, +-1000, +-30000 through the bias, rows leading by 256 and
    8192 with the label on the lead and on the smallest logit, flat rows: all
    finite; loss (rtol 1e-5, atol 1e-6), db (rtol 1e-4, atol 1e-7) and dW
    (1e-4 |ref| + 1e-7 max|x| of its column) against fp64 cross-entropy of the
    fp32 logits fl(a W + b); the offset-0 problem also without a bias."""
    M = past_workgroups() if M == "big" else M
    p = xp.softmax_edge_step(M, C, xp.edge_seed(M, C))
    Xd, Wd = p.X.to(dtype).to(DEV), p.W.to(DEV)
    failed = {}
    for off, bias, labels in xp.edge_variants():
        c = xp.edge_case(p, off, bias=bias, labels=labels)
        got = raw_step(Xd, Wd, c.b.to(DEV) if bias else None, c.y.to(DEV))
        bad = xp.check_edge(p, c, got)
        dl = float((got[0].double().cpu() - c.loss).abs())
        ddw = float((got[1].double().cpu() - c.dW).abs().max())
        ddb = float((got[2].double().cpu() - c.db).abs().max()) if bias else float("nan")
        name = xp.edge_name(M, C, off, bias, labels, dtype)
        print(f"xent x16 {name}: loss {float(c.loss):.6g} |dloss| {dl:.3e}, max |ddb| {ddb:.3e}, "
              f"max |ddW| {ddw:.3e}")
        if bad:
            failed[name] = bad
    assert failed == {}


# ---- 3. the fused loops on an edge problem ------------------------------------------

@DT
def test_loops_first_loss_has_the_raw_steps_bits(dtype, monkeypatch):
    """M = 1000, C = 41, offset +30000: the first loss sgc_train_adam_x16
    (epochs = 1) and sgc_train_lbfgs_x16 (steps = 1, max_iter = 1) report is
    the raw step's, bit for bit -- the stop-aware launch A and
    xent16_reduce_kernel<true> are compiled instances of their own."""
    from sgc_amd.optim import LBFGS
    from test_gpu_train_x16 import Run, count_calls, sgc_model
    M, C = 1000, 41
    p = xp.softmax_edge_step(M, C, xp.edge_seed(M, C))
    c = xp.edge_case(p, 30000.0)
    Xd, yd = p.X.to(dtype).to(DEV), c.y.to(DEV)
    raw = raw_step(Xd, p.W.to(DEV), c.b.to(DEV), yd)
    assert xp.check_edge(p, c, raw) == []
    adam = Run(Xd, p.W, c.b, yd).train(1).result()
    assert adam["loss"].shape == (1,) and same_bits(adam["loss"][0], raw[0])
    model = sgc_model(p.K, C, p.W.to(DEV), c.b.to(DEV))
    opt = LBFGS(model.parameters(), lr=1, max_iter=1)
    calls = count_calls(monkeypatch, "sgc_train_lbfgs_x16")
    losses = opt.run_steps(model, Xd, yd, 1)
    torch.cuda.synchronize()
    assert calls == ["sgc_train_lbfgs_x16"]
    assert losses.shape == (1,) and same_bits(losses[0], raw[0])
    print(f"xent x16 loops {IDS[dtype]}: first loss {float(raw[0])!r} in all three")


# ---- 4. the top of the pitch range ---------------------------------------------------

@DT
def test_top_of_the_pitch_range(dtype):
    """X = the first 66 columns of a [1023, 2^20] 16-bit buffer (2 GiB, only
    those columns written): M * ldx * 2 = 2,145,386,496 < 2^31 - 1, one step
    below the refusal test_classifier_x16_cpu.py shows.  The forward and the
    weight backward are bit-exact on integer operands, the fused step meets its
    fp64 tolerances and gets the integer-operand loss to 1 ulp."""
    from sgc_amd import _lib
    from sgc_amd.propagate import X16_DTYPES, linear, linear_backward
    lib = _lib.load()
    M, ldx, K, C = 1023, 1 << 20, 66, 17
    assert M * ldx * 2 == 2145386496 < 2 ** 31 - 1
    buf = torch.empty((M, ldx), dtype=dtype, device=DEV)
    X = buf[:, :K]
    try:
        assert X.stride(0) == ldx
        dt = X16_DTYPES[dtype]
        for fn, word in ((lib.sgc_linear_x16_kernel_name, b"linear_x16_kernel"),
                         (lib.sgc_linear_backward_x16_kernel_name, b"xent_dw_cols_x16_kernel"),
                         (lib.sgc_linear_xent_x16_kernel_name, b"xent_fwd_x16_kernel")):
            assert fn(M, K, ldx, C, _lib.ptr(X), dt).startswith(word)
            assert fn(M + 1, K, ldx, C, _lib.ptr(X), dt) == b"none"  # 2^31: refused
        bits, wide = (10, "w") if dtype == torch.bfloat16 else (10, "x")
        # forward, integer operands
        Xi, W, b = p16.integer_operands_x16(M, K, C, bits, cp.case_seed(M, K, C), dtype, wide=wide)
        X.copy_(Xi)
        ref = F_.linear(Xi.double(), W.double(), b.double()).float()
        assert torch.equal(linear(X, W.to(DEV), b.to(DEV)).cpu(), ref)
        # weight backward, integer operands
        Xi, dY = p16.integer_operands_x16(M, K, C, bits, cp.case_seed(M, K, C) + 1, dtype,
                                          backward=True, wide=wide)
        X.copy_(Xi)
        dW, db = linear_backward(X, dY.to(DEV))
        assert torch.equal(dW.cpu(), (dY.double().t() @ Xi.double()).float())
        assert torch.equal(db.cpu(), dY.double().sum(0).float())
        # the fused step: the sparse-ish problem against fp64, integer operands to 1 ulp
        Xs, W, b, y = problem(M, K, C)
        X.copy_(Xs.to(dtype))
        Wd, bd, yd = W.to(DEV), b.to(DEV), y.to(DEV)
        rl, rW, rb = xent_grads(X.double(), Wd.double(), bd.double(), yd)
        loss, dW, db = raw_step(X, Wd, bd, yd)
        torch.testing.assert_close(loss.double(), rl, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(dW.double(), rW, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(db.double(), rb, rtol=1e-4, atol=1e-6)
        Xs, W, b, y = problem(M, K, C, ints=True)
        assert torch.equal(Xs.to(dtype).float(), Xs)
        X.copy_(Xs.to(dtype))
        Wd, bd, yd = W.to(DEV), b.to(DEV), y.to(DEV)
        rl = xent_grads(X.double(), Wd.double(), bd.double(), yd)[0]
        loss = raw_step(X, Wd, bd, yd)[0]
        want = rl.float()
        ulp = float(torch.nextafter(want, want + 1) - want)
        print(f"xent x16 pitch 2^20 {IDS[dtype]}: integer loss {float(loss)!r} fp64 {float(rl)!r} "
              f"ulp {ulp:.3e}")
        assert abs(float(loss) - float(rl)) <= ulp
    finally:
        del buf, X
        torch.cuda.empty_cache()
