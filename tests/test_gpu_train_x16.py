"""The fused training loops on 16-bit features on the GPU.

L-BFGS (LBFGS.run_steps / sgc_train_lbfgs_x16): the oracle is exact.  The
stepwise device optimiser whose closure calls propagate.linear_xent(X16, W, b,
y) and assigns .grad runs the same three launches of sgc_linear_xent_x16 and
the same iterate kernel, so the fused run must equal it bit for bit -- W, b,
the whole device state, every status and every loss.

Adam (sgc_train_adam_x16): tests/test_gpu_adam.py's bound -- our error against
ref_train on X16.double() is at most twice that of torch's fp32 loop on
X16.float(), plus FLOOR -- and run_epochs' contract on 16-bit features."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adam_ref import BETAS, EPS, FLOOR, LR, ref_train, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
WD = 5e-4
DTYPES = (torch.bfloat16, torch.float16)
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# --- L-BFGS ----------------------------------------------------------------------------

def lbfgs_problem(M, K, C, dtype, layout="contiguous", seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g).to(dtype)
    y = torch.randint(0, C, (M,), generator=g)
    if layout == "strided":  # ldx = K + 6
        buf = torch.zeros((M, K + 6), dtype=dtype, device=DEV)
        buf[:, :K].copy_(X)
        X = buf[:, :K]
    else:
        X = X.to(DEV)
    return X, y.to(DEV)


def models(K, C, n=2, seed=1):
    from sgc_amd.models import SGC
    torch.manual_seed(seed)
    ms = [SGC(K, C).to(DEV) for _ in range(n)]
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    return ms


def stepwise(model, X, y, steps, **opts):
    """`steps` step() calls of the device optimiser; the closure is the fused
    16-bit step, its dW / db assigned as the gradients."""
    from sgc_amd.optim import LBFGS
    from sgc_amd.propagate import linear_xent
    opt = LBFGS(model.parameters(), **opts)
    assert opt.device_path()

    def closure():
        loss, dW, db = linear_xent(X, model.W.weight, model.W.bias, y)
        model.W.weight.grad, model.W.bias.grad = dW, db
        return loss
    statuses, losses = [], []
    for _ in range(steps):
        losses.append(opt.step(closure).detach())
        statuses.append(opt.last_status)
    return opt, statuses, torch.stack(losses)


def fused(model, X, y, steps, **opts):
    from sgc_amd.optim import LBFGS
    opt = LBFGS(model.parameters(), **opts)
    losses = opt.run_steps(model, X, y, steps)
    assert all(p.grad is None for p in model.parameters())
    return opt, opt.step_statuses, losses


def assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2):
    assert s1 == s2, (s1, s2)
    assert same_bits(l1, l2), (l1, l2)
    assert same_bits(m1.W.weight.detach(), m2.W.weight.detach())
    assert same_bits(m1.W.bias.detach(), m2.W.bias.detach())
    assert torch.equal(o1._dev_state, o2._dev_state)
    assert o1.last_status == o2.last_status


def count_calls(monkeypatch, name):
    from sgc_amd import _lib
    lib = _lib.load()
    real = getattr(lib, name)
    calls = []

    def counted(*args):
        calls.append(name)
        return real(*args)
    monkeypatch.setattr(lib, name, counted)
    return calls


LBFGS_SHAPES = [(1, 2, 1), (70, 34, 3), (257, 64, 7), (300, 602, 41), (300, 40, 48),
                (3000, 602, 41)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
@pytest.mark.parametrize("M,K,C", LBFGS_SHAPES)
def test_run_steps_bit_equal_to_the_stepwise_run(M, K, C, layout, dtype, monkeypatch):
    X, y = lbfgs_problem(M, K, C, dtype, layout)
    m1, m2 = models(K, C)
    opts = dict(max_iter=4)
    o1, s1, l1 = stepwise(m1, X, y, 2, **opts)
    calls = count_calls(monkeypatch, "sgc_train_lbfgs_x16")
    o2, s2, l2 = fused(m2, X, y, 2, **opts)
    torch.cuda.synchronize()
    assert calls == ["sgc_train_lbfgs_x16"]
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2)
    assert all(s[3] >= 1 for s in s2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_stop_mid_step_and_next_steps_reset(dtype):
    """max_eval = 2 stops each step on its second closure: the stop-aware
    launches of the remaining closures run after the stop and move nothing; a
    loose tolerance_grad stops at entry; fused and stepwise steps alternate."""
    from test_lbfgs_host import STOP_MAX_EVAL, STOP_OPT_AT_ENTRY
    X, y = lbfgs_problem(70, 34, 3, dtype)
    m1, m2 = models(34, 3)
    opts = dict(max_iter=6, max_eval=2)
    o1, s1, l1 = stepwise(m1, X, y, 3, **opts)
    o2, s2, l2 = fused(m2, X, y, 3, **opts)
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2)
    assert [s[4] for s in s2] == [STOP_MAX_EVAL] * 3 and s2[1][3] == 2
    m1, m2 = models(34, 3)
    opts = dict(max_iter=4, tolerance_grad=10.0)
    o1, s1, l1 = stepwise(m1, X, y, 2, **opts)
    o2, s2, l2 = fused(m2, X, y, 2, **opts)
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2)
    assert [s[4] for s in s2] == [STOP_OPT_AT_ENTRY] * 2
    # one state, fused and stepwise steps in turn
    from sgc_amd.optim import LBFGS
    from sgc_amd.propagate import linear_xent
    m1, m2 = models(34, 3)
    o1, s1, l1 = stepwise(m1, X, y, 3, max_iter=4)
    o2 = LBFGS(m2.parameters(), max_iter=4)

    def closure():
        loss, dW, db = linear_xent(X, m2.W.weight, m2.W.bias, y)
        m2.W.weight.grad, m2.W.bias.grad = dW, db
        return loss
    s2, l2 = [], []
    l2.append(o2.run_steps(m2, X, y, 1)[0])
    s2.append(o2.last_status)
    l2.append(o2.step(closure).detach())
    s2.append(o2.last_status)
    for p in m2.parameters():
        p.grad = None
    l2.append(o2.run_steps(m2, X, y, 1)[0])
    s2.append(o2.last_status)
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, torch.stack(l2))


def test_lbfgs_end_to_end_like_torch():
    """test_classifier_end_to_end_like_torch's shape and bound on bf16
    features, against torch.optim.LBFGS on X.float()."""
    from sgc_amd.optim import LBFGS
    torch.manual_seed(0)
    X = torch.randn(3000, 602, device=DEV).bfloat16()
    Xf = X.float()
    y = torch.randint(0, 41, (3000,), device=DEV)
    m1, m2 = models(602, 41, seed=0)
    ours = LBFGS(m1.parameters(), lr=1)
    ours.run_steps(m1, X, y, 2)
    assert all(p.grad is None for p in m1.parameters())  # the fused path ran
    theirs = torch.optim.LBFGS(m2.parameters(), lr=1)

    def closure():
        theirs.zero_grad()
        loss = F.cross_entropy(m2(Xf), y)
        loss.backward()
        return loss
    for _ in range(2):
        theirs.step(closure)
    losses = [F.cross_entropy(m(Xf), y).item() for m in (m1, m2)]
    a, b = ours.state[ours._params[0]], theirs.state[theirs._params[0]]
    print("fused lbfgs x16 end to end: losses", losses, "n_iter/func_evals",
          (a["n_iter"], a["func_evals"]), (b["n_iter"], b["func_evals"]))
    assert (a["n_iter"], a["func_evals"]) == (b["n_iter"], b["func_evals"])
    assert abs(losses[0] - losses[1]) <= 1e-3 * max(1.0, abs(losses[1])), losses


def test_run_steps_is_one_call_and_one_read_back(monkeypatch):
    import sgc_amd.optim as so
    X, y = lbfgs_problem(257, 64, 7, torch.bfloat16)
    (m,) = models(64, 7, n=1)
    opt = so.LBFGS(m.parameters(), max_iter=6)
    opt.run_steps(m, X, y, 1)  # builds the state, checks the labels once
    torch.cuda.synchronize()
    calls = {"sync": 0, "item": 0, "float": 0, "read": 0, "step_read": 0}

    def counted(key, fn):
        def w(*args, **kw):
            calls[key] += 1
            return fn(*args, **kw)
        return w
    monkeypatch.setattr(torch.cuda, "synchronize", counted("sync", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "__float__", counted("float", torch.Tensor.__float__))
    monkeypatch.setattr(so, "_read_status_trace", counted("read", so._read_status_trace))
    monkeypatch.setattr(so, "_read_status", counted("step_read", so._read_status))
    native = count_calls(monkeypatch, "sgc_train_lbfgs_x16")
    opt.run_steps(m, X, y, 2)
    monkeypatch.undo()
    assert calls == {"sync": 0, "item": 0, "float": 0, "read": 1, "step_read": 0}, calls
    assert native == ["sgc_train_lbfgs_x16"]
    assert all(p.grad is None for p in m.parameters())
    assert len(opt.step_statuses) == 2 and opt.step_statuses[-1] == opt.last_status


def test_odd_pitch_still_runs_the_literal_loop(monkeypatch):
    """bf16 at K = 33 (an odd pitch): no re-pitching copy, the literal loop,
    bit for bit -- the pinned fallback of test_gpu_lbfgs_train.py."""
    from sgc_amd.optim import LBFGS
    X, y = lbfgs_problem(70, 33, 3, torch.bfloat16)
    m1, m2 = models(33, 3)

    def literal(opt, model):
        def closure():
            opt.zero_grad()
            loss = F.cross_entropy(model(X), y)
            loss.backward()
            return loss
        losses, statuses = [], []
        for _ in range(2):
            losses.append(opt.step(closure).detach())
            statuses.append(opt.last_status)
        return torch.stack(losses), statuses
    o1 = LBFGS(m1.parameters(), max_iter=4)
    want, statuses = literal(o1, m1)
    o2 = LBFGS(m2.parameters(), max_iter=4)
    native = count_calls(monkeypatch, "sgc_train_lbfgs_x16")
    got = o2.run_steps(m2, X, y, 2)
    assert native == []
    assert same_bits(got, want) and o2.step_statuses == statuses
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert same_bits(p.detach(), q.detach())
    assert torch.equal(o1._dev_state, o2._dev_state)


# --- Adam ------------------------------------------------------------------------------

def adam_problem(M, K, C, seed=1):
    """tests/test_gpu_adam.py's sparse-ish citation-like features."""
    gen = torch.Generator().manual_seed(seed + 31 * M + K)
    y = torch.randint(0, C, (M,), generator=gen)
    cent = torch.randn(C, K, generator=gen) * 0.05
    X = (torch.rand(M, K, generator=gen) < 0.01).float() * 0.1 + cent[y].abs() * 0.2
    W = (torch.rand(C, K, generator=gen) * 2 - 1) / math.sqrt(K)
    b = (torch.rand(C, generator=gen) * 2 - 1) / math.sqrt(K)
    return X, W, b, y


def torch_loop32(X, W, b, y, epochs, lr, wd):
    """torch's own fp32 loop on the device: autograd + torch.optim.Adam."""
    W = W.to(DEV).clone().requires_grad_(True)
    b = None if b is None else b.to(DEV).clone().requires_grad_(True)
    params = [W] + ([] if b is None else [b])
    opt = torch.optim.Adam(params, lr=lr, weight_decay=wd)
    losses = []
    for _ in range(epochs):
        opt.zero_grad()
        loss = F.cross_entropy(F.linear(X, W, b), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    out = dict(W=W.detach(), mW=opt.state[W]["exp_avg"], vW=opt.state[W]["exp_avg_sq"],
               loss=torch.stack(losses))
    if b is not None:
        out.update(b=b.detach(), mb=opt.state[b]["exp_avg"], vb=opt.state[b]["exp_avg_sq"])
    return out


class Run:
    """Device buffers of one training problem and calls of sgc_train_adam_x16."""

    def __init__(self, X16, W, b, y):
        from sgc_amd import _lib
        from sgc_amd.propagate import X16_DTYPES
        self.lib = _lib.load()
        self.X, self.y = X16, y
        self.dt = X16_DTYPES[X16.dtype]
        self.W = W.to(DEV).clone()
        self.b = None if b is None else b.to(DEV).clone()
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb = None if b is None else torch.zeros_like(self.b)
        self.vb = None if b is None else torch.zeros_like(self.b)
        (self.M, self.K), self.C = X16.shape, W.shape[0]
        nbytes = self.lib.sgc_train_adam_x16_workspace(self.M, self.K, self.C)
        assert nbytes > 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.step = 0
        self.losses = []

    def train(self, epochs, lr=LR, wd=WD):
        from sgc_amd import _lib
        trace = torch.empty(epochs, device=DEV)
        _lib.check(self.lib.sgc_train_adam_x16(
            _lib.ptr(self.X), self.dt, self.X.stride(0), _lib.ptr(self.W), _lib.ptr(self.b),
            _lib.ptr(self.y), self.M, self.K, self.C, _lib.ptr(self.mW), _lib.ptr(self.vW),
            _lib.ptr(self.mb), _lib.ptr(self.vb), self.step, epochs, lr, BETAS[0], BETAS[1], EPS,
            wd, _lib.ptr(trace), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_handle(DEV)),
            "train_adam_x16")
        self.step += epochs
        self.losses.append(trace)
        return self

    def result(self):
        torch.cuda.synchronize()
        out = dict(W=self.W, mW=self.mW, vW=self.vW, loss=torch.cat(self.losses))
        if self.b is not None:
            out.update(b=self.b, mb=self.mb, vb=self.vb)
        return out


def check_bound(errs, what):
    for k, (ours, t32) in errs.items():
        print(f"adam x16 {what}: {k}: e(ours)={ours:.3e} e(torch fp32)={t32:.3e}")
    for k, (ours, t32) in errs.items():
        assert ours <= 2 * t32 + FLOOR, (what, k, ours, t32)


def errors(got, ref, t32):
    return {k: (rel_err(got[k], ref[k]), rel_err(t32[k], ref[k])) for k in got}


_refs = {}


def references(M, K, C, dtype, epochs=3, bias=True):
    """(X16 on the device in an even pitch, W, b, y), ref_train's fp64 result on
    X16.double(), torch's fp32 loop on X16.float() -- computed once."""
    key = (M, K, C, dtype, epochs, bias)
    if key not in _refs:
        X, W, b, y = adam_problem(M, K, C)
        if not bias:
            b = None
        X16 = X.to(dtype)
        buf = torch.zeros((M, K + (K & 1)), dtype=dtype, device=DEV)  # 1433 -> pitch 1434
        buf[:, :K].copy_(X16)
        Xd, yd = buf[:, :K], y.to(DEV)
        ref = ref_train(Xd.double(), W.to(DEV), None if b is None else b.to(DEV), yd, epochs, LR,
                        WD)
        t32 = torch_loop32(Xd.float(), W, b, yd, epochs, LR, WD)
        _refs[key] = ((Xd, W, b, yd), ref, t32)
    return _refs[key]


ADAM_SHAPES = [(1, 2, 1), (60, 500, 3), (140, 1433, 7), (37, 66, 17), (314, 64, 41),
               (3000, 602, 41)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", ADAM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_train_adam_against_ref_train(shape, dtype):
    prob, ref, t32 = references(*shape, dtype)
    got = Run(*prob).train(3).result()
    check_bound(errors(got, ref, t32), "train %s %s" % (shape, IDS[dtype]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_train_adam_variants(dtype):
    """No bias; 3 epochs in one call = three calls of one (step0 continues);
    two runs give the same bits; adam_kernel = 2 still runs, on the general
    schedule."""
    from sgc_amd import _lib
    lib = _lib.load()
    shape = (37, 66, 17)
    prob, ref, t32 = references(*shape, dtype, bias=False)
    check_bound(errors(Run(*prob).train(3).result(), ref, t32), "no bias")
    prob, ref, t32 = references(*shape, dtype)
    one = Run(*prob).train(3).result()
    run = Run(*prob).train(1).train(1).train(1)
    assert run.step == 3
    thrice = run.result()
    again = Run(*prob).train(3).result()
    for k in one:
        assert torch.equal(one[k], thrice[k]), k
        assert torch.equal(one[k], again[k]), k
    assert lib.sgc_set_tuning(b"adam_kernel", 2) == 0
    try:
        small = Run(*prob).train(3).result()
        assert lib.sgc_get_tuning(b"adam_kernel_last") == 1
    finally:
        lib.sgc_set_tuning(b"adam_kernel", 0)
    for k in one:
        assert torch.equal(one[k], small[k]), k


def sgc_model(K, C, W, b):
    from sgc_amd.models import SGC
    m = SGC(K, C).to(DEV)
    with torch.no_grad():
        m.W.weight.copy_(W)
        m.W.bias.copy_(b)
    return m


@pytest.mark.parametrize("K", [64, 65])
def test_run_epochs_is_one_call_and_leaves_grad_none(K, monkeypatch):
    """K = 65: a contiguous odd pitch -- one even-pitch copy, still one call."""
    from sgc_amd.optim import Adam
    M, C = 60, 3
    X, W, b, y = adam_problem(M, K, C)
    model = sgc_model(K, C, W, b)
    Xd, yd = X.to(DEV).bfloat16(), y.to(DEV)
    opt = Adam(model.parameters(), lr=LR, weight_decay=WD)
    calls = count_calls(monkeypatch, "sgc_train_adam_x16")
    out = opt.run_epochs(model, Xd, yd, 5)
    assert calls == ["sgc_train_adam_x16"]
    assert all(p.grad is None for p in model.parameters())
    assert out.dim() == 0 and bool(torch.isfinite(out))
    assert float(opt.state[model.W.weight]["step"]) == 5.0
    # the trace and the weights: the raw call's on the same features
    ref = Run(Xd if K % 2 == 0 else references_even(Xd), W, b, yd).train(5).result()
    assert torch.equal(ref["W"], model.W.weight.detach())
    assert torch.equal(ref["loss"][-1], out)


def references_even(X16):
    buf = torch.zeros((X16.shape[0], X16.shape[1] + 1), dtype=X16.dtype, device=DEV)
    buf[:, :-1].copy_(X16)
    return buf[:, :-1]


# --- drivers -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bfloat16", "float16"])
def test_reddit_driver_fused_lbfgs_on_16_bit_features(name, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(HERE), "drivers"))
    import reddit
    calls = count_calls(monkeypatch, "sgc_train_lbfgs_x16")
    f1, _, _ = reddit.main(["--synthetic", "3000", "--feature-dtype", name, "--fused-lbfgs"])
    assert calls == ["sgc_train_lbfgs_x16"]
    assert np.isfinite(float(f1)) and 0.0 <= float(f1) <= 1.0


@pytest.mark.parametrize("name", ["bfloat16", "float16"])
def test_citation_driver_device_adam_on_16_bit_features(name, tmp_path, monkeypatch):
    from planetoid_synth import write_planetoid
    with open(os.path.join(HERE, "golden", "e2e_citation.json")) as f:
        golden = json.load(f)
    write_planetoid(str(tmp_path), **golden["dataset"])
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(HERE), "drivers"))
    import citation
    calls = count_calls(monkeypatch, "sgc_train_adam_x16")
    acc_val, acc_test = citation.main(["--dataset", "synth", "--epochs", "20", "--degree", "2",
                                       "--feature-dtype", name, "--device-adam"])
    assert calls == ["sgc_train_adam_x16"]
    assert np.isfinite(acc_val) and np.isfinite(acc_test) and 0.0 <= acc_test <= 1.0
