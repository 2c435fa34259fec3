"""sgc_amd.optim.Adam on the GPU: one sgc_adam_step_f32 launch against the
fp64 restatement (tests/adam_ref.py, validated against torch.optim.Adam in
tests/test_adam_host.py) and against torch's fp32 ops on the device, the whole
loop (sgc_train_adam_f32) on both schedules and the auto rule against
`ref_train` and torch's fp32 loop, determinism, and run_epochs' contract.

The bound is tests/test_gpu_lbfgs.py's: our error against the fp64 value is at
most twice that of torch's fp32 arithmetic on the same inputs on the device,
plus FLOOR (four fp32 epsilons); both are printed."""
import contextlib
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from adam_ref import (BETAS, EPS, FLOOR, LR, ONE_STEP_CASES, adam_math, one_step_case,
                      one_step_errors, ref_train, rel_err)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIMIT = 313  # the small schedule's row limit (include/sgc_amd.h)
WD = 5e-4


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import _lib
    lib = _lib.load()
    assert lib.sgc_get_tuning(b"adam_small_max_rows") == LIMIT
    return lib


@contextlib.contextmanager
def knob(lib, value):
    assert lib.sgc_set_tuning(b"adam_kernel", value) == 0
    try:
        yield
    finally:
        lib.sgc_set_tuning(b"adam_kernel", 0)


def check_bound(errs, what):
    for k, (ours, t32) in errs.items():
        print(f"adam {what}: {k}: e(ours)={ours:.3e} e(torch fp32)={t32:.3e}")
    for k, (ours, t32) in errs.items():
        assert ours <= 2 * t32 + FLOOR, (what, k, ours, t32)


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def dev_step(lib, ps, gs, ms, vs, step, wd):
    from sgc_amd import _lib
    n = len(ps)
    _lib.check(lib.sgc_adam_step_f32(n, ptrs(ps), ptrs(gs), ptrs(ms), ptrs(vs),
                                     (ctypes.c_int64 * n)(*[p.numel() for p in ps]), step, LR,
                                     BETAS[0], BETAS[1], EPS, wd, _lib.stream_handle(DEV)),
               "adam_step_f32")


# --- one step ------------------------------------------------------------------------

def torch32(p, g, m, v, step, wd):
    return adam_math(p.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV), step, LR, wd)


@pytest.mark.parametrize("case", ONE_STEP_CASES, ids=lambda c: "n%d-step%d-wd%g-%s" % c)
def test_one_step(lib, case):
    def ours(p, g, m, v, step, wd):
        p, g, m, v = (t.to(DEV) for t in (p, g, m, v))
        dev_step(lib, [p], [g], [m], [v], step, wd)
        return p, m, v
    e_ours = one_step_errors(case, ours)
    e_t32 = one_step_errors(case, torch32)
    check_bound({k: (e_ours[k], e_t32[k]) for k in "pmv"}, "one step %s" % (case,))
    n, step, wd, edge = case
    a, b = (ours(*one_step_case(n, step, wd, edge), step, wd) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))  # two runs: the same bits


@pytest.mark.parametrize("step,wd", [(1, 0.0), (10000, WD)])
def test_one_step_unaligned_tensors_and_a_skipped_one(lib, step, wd):
    """Three tensors at 4-B-only aligned offsets of one buffer and a fourth
    whose gradient is NULL, in one launch."""
    sizes, offs = (63, 1025, 4097, 65), (1, 67, 1095, 5195)
    total = offs[-1] + sizes[-1] + 3
    cases = [one_step_case(n, step, wd, seed=7 + i) for i, n in enumerate(sizes)]
    bufs = [torch.full((total,), 7.0, device=DEV) for _ in range(4)]  # p, g, m, v
    views = [[buf[o:o + n] for o, n in zip(offs, sizes)] for buf in bufs]
    for i, c in enumerate(cases):
        for k in range(4):
            views[k][i].copy_(c[k])
            assert i == 3 or views[k][i].data_ptr() % 8 == 4
    before = [buf.clone() for buf in bufs]
    gs = views[1][:3] + [None]
    dev_step(lib, views[0], gs, views[2], views[3], step, wd)
    torch.cuda.synchronize()
    for i in range(3):
        c = cases[i]
        ref = adam_math(*(t.double() for t in c), step, LR, wd)
        t32 = torch32(*c, step, wd)
        got = (views[0][i], views[2][i], views[3][i])
        check_bound({k: (rel_err(got[j], ref[j]), rel_err(t32[j], ref[j]))
                     for j, k in enumerate("pmv")}, f"unaligned tensor {i} step {step}")
    # the skipped tensor and every element between the tensors: bit-unchanged
    touched = torch.zeros(total, dtype=torch.bool, device=DEV)
    for o, n in zip(offs[:3], sizes[:3]):
        touched[o:o + n] = True
    for k in (0, 2, 3):
        assert torch.equal(bufs[k][~touched], before[k][~touched])
    assert torch.equal(bufs[1], before[1])


# --- the whole loop --------------------------------------------------------------------

def problem(M, K, C, seed=1, ints=False):
    """scripts' sparse-ish citation-like features (or small integers)."""
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


def torch_loop32(X, W, b, y, epochs, lr, wd):
    """torch's own fp32 loop on the device: autograd + torch.optim.Adam."""
    X, y = X.to(DEV), y.to(DEV)
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
    """Device buffers of one training problem and calls of sgc_train_adam_f32."""

    def __init__(self, lib, X, W, b, y, pad=0):
        self.lib = lib
        M, K = X.shape
        if pad:  # ldx = K + pad on a base that is only 4-B aligned
            flat = torch.zeros(1 + M * (K + pad), device=DEV)
            self.X = flat[1:].view(M, K + pad)[:, :K]
            self.X.copy_(X)
            assert self.X.data_ptr() % 8 == 4 and self.X.stride(0) == K + pad
        else:
            self.X = X.to(DEV)
        self.y = y.to(DEV)
        self.W = W.to(DEV).clone()
        self.b = None if b is None else b.to(DEV).clone()
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb = None if b is None else torch.zeros_like(self.b)
        self.vb = None if b is None else torch.zeros_like(self.b)
        self.M, self.K, self.C = M, K, W.shape[0]
        nbytes = lib.sgc_train_adam_workspace(M, K, self.C)
        assert nbytes > 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.step = 0
        self.losses = []

    def train(self, epochs, lr=LR, wd=WD):
        from sgc_amd import _lib
        trace = torch.empty(epochs, device=DEV)
        _lib.check(self.lib.sgc_train_adam_f32(
            _lib.ptr(self.X), self.X.stride(0), _lib.ptr(self.W), _lib.ptr(self.b), _lib.ptr(self.y),
            self.M, self.K, self.C, _lib.ptr(self.mW), _lib.ptr(self.vW), _lib.ptr(self.mb),
            _lib.ptr(self.vb), self.step, epochs, lr, BETAS[0], BETAS[1], EPS, wd, _lib.ptr(trace),
            _lib.ptr(self.ws), self.ws.numel(), _lib.stream_handle(DEV)), "train_adam_f32")
        self.step += epochs
        self.losses.append(trace)
        return self

    def result(self):
        torch.cuda.synchronize()
        out = dict(W=self.W, mW=self.mW, vW=self.vW, loss=torch.cat(self.losses))
        if self.b is not None:
            out.update(b=self.b, mb=self.mb, vb=self.vb)
        return out


_refs = {}


def references(M, K, C, epochs=3, bias=True):
    """(problem, ref_train's fp64 result, torch's fp32 loop), computed once."""
    key = (M, K, C, epochs, bias)
    if key not in _refs:
        X, W, b, y = problem(M, K, C)
        if not bias:
            b = None
        _refs[key] = ((X, W, b, y), ref_train(X, W, b, y, epochs, LR, WD),
                      torch_loop32(X, W, b, y, epochs, LR, WD))
    return _refs[key]


def errors(got, ref, t32):
    return {k: (rel_err(got[k], ref[k]), rel_err(t32[k], ref[k])) for k in got}


SMALL_OK = [(1, 1, 1), (60, 500, 3), (140, 1433, 7), (120, 3703, 6), (37, 65, 17), (LIMIT, 64, 64)]
PAST_LIMIT = (LIMIT + 1, 63, 41)
# every shape under every setting, and two more on the general schedule only
TRAIN_CASES = [(s, k) for s in SMALL_OK + [PAST_LIMIT] for k in (1, 2, 0)] + \
    [((129, 602, 41), 1), ((3000, 602, 41), 1)]


@pytest.mark.parametrize("shape,setting", TRAIN_CASES,
                         ids=lambda v: "%dx%dx%d" % v if isinstance(v, tuple) else
                         ["auto", "general", "small"][v])
def test_train_against_ref_train(lib, shape, setting):
    prob, ref, t32 = references(*shape)
    with knob(lib, setting):
        got = Run(lib, *prob).train(3).result()
        last = lib.sgc_get_tuning(b"adam_kernel_last")
    if shape == PAST_LIMIT or setting == 1:
        assert last == 1  # (past the row limit: general under every setting)
    elif setting == 2:
        assert last == 2
    elif shape in ((60, 500, 3), (140, 1433, 7), (120, 3703, 6)):
        assert last == 2  # the auto rule takes the small schedule at the citation shapes
    else:
        assert last in (1, 2)
    check_bound(errors(got, ref, t32), "train %s adam_kernel=%d (ran %d)" % (shape, setting, last))


@pytest.mark.parametrize("setting", [1, 2], ids=["general", "small"])
def test_train_variants(lib, setting):
    """No bias; ldx = K + 3 on a 4-B aligned base; step0 = 7 continuing a
    previous call; 3 epochs in one call = three calls of one; two runs."""
    shape = (37, 65, 17)
    with knob(lib, setting):
        prob, ref, t32 = references(*shape, bias=False)
        check_bound(errors(Run(lib, *prob).train(3).result(), ref, t32), "no bias")
        prob, ref, t32 = references(*shape)
        one = Run(lib, *prob).train(3).result()
        padded = Run(lib, *prob, pad=3).train(3).result()
        check_bound(errors(padded, ref, t32), "ldx = K + 3")
        thrice = Run(lib, *prob).train(1).train(1).train(1).result()
        again = Run(lib, *prob).train(3).result()
        for k in one:
            assert torch.equal(one[k], thrice[k]), k
            assert torch.equal(one[k], again[k]), k
            assert torch.equal(one[k], padded[k]), k
        prob, ref, t32 = references(*shape, epochs=10)
        run = Run(lib, *prob).train(7)
        assert run.step == 7
        cont = run.train(3).result()
        whole = Run(lib, *prob).train(10).result()
        for k in cont:
            assert torch.equal(cont[k], whole[k]), k
        check_bound(errors(cont, ref, t32), "step0 = 7 continuing")


@pytest.mark.parametrize("setting", [1, 2], ids=["general", "small"])
@pytest.mark.parametrize("shape", [(60, 500, 3), (140, 1433, 7), (120, 3703, 6), (37, 65, 17)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_integer_operands_first_loss(lib, shape, setting):
    """Small-integer X, W and b give exact logits on every path: the first
    loss equals the fp64 value to 1 ulp (a dropped or doubled K block moves
    it by far more); lr = 0 leaves the weights where they were."""
    X, W, b, y = problem(*shape, ints=True)
    ref = ref_train(X, W, b, y, 1, 0.0, 0.0)
    with knob(lib, setting):
        got = Run(lib, X, W, b, y).train(1, lr=0.0, wd=0.0).result()
    want = ref["loss"][0].float()
    ulp = float(torch.nextafter(want, want + 1) - want)
    print(f"integer probe {shape} adam_kernel={setting}: loss {float(got['loss'][0])!r} "
          f"fp64 {float(ref['loss'][0])!r} ulp {ulp:.3e}")
    assert abs(float(got["loss"][0]) - float(ref["loss"][0])) <= ulp
    assert torch.equal(got["W"].cpu(), W) and torch.equal(got["b"].cpu(), b)


# --- run_epochs ---------------------------------------------------------------------------

def sgc_pair(K, C, W, b):
    from sgc_amd.models import SGC
    models = []
    for _ in range(2):
        m = SGC(K, C).to(DEV)
        with torch.no_grad():
            m.W.weight.copy_(W)
            m.W.bias.copy_(b)
        models.append(m)
    return models


@pytest.mark.parametrize("setting", [0, 1, 2], ids=["auto", "general", "small"])
def test_hundred_epochs_like_torch(lib, setting):
    """100 epochs at the Cora train shape on sparse-ish features (lr 0.2,
    weight decay 5e-6): the final loss within 1e-3 max(1, |loss|) of torch's
    fp32 loop (test_classifier_end_to_end_like_torch's bound), equal train
    accuracy; the W errors against ref_train are printed, not asserted."""
    from sgc_amd.optim import Adam
    M, K, C = 140, 1433, 7
    X, W, b, y = problem(M, K, C)
    key = ("hundred",)
    if key not in _refs:
        _refs[key] = (ref_train(X, W, b, y, 100, 0.2, 5e-6), torch_loop32(X, W, b, y, 100, 0.2, 5e-6))
    ref, t32 = _refs[key]
    model = sgc_pair(K, C, W, b)[0]
    Xd, yd = X.to(DEV), y.to(DEV)
    opt = Adam(model.parameters(), lr=0.2, weight_decay=5e-6)
    with knob(lib, setting):
        trace = opt.run_epochs(model, Xd, yd, 100, loss_trace=True)
    assert trace.shape == (100,) and model.W.weight.grad is None
    loss, loss_t = float(trace[-1]), float(t32["loss"][-1])
    print(f"100 epochs adam_kernel={setting}: loss ours {loss:.6f} torch {loss_t:.6f} fp64 "
          f"{float(ref['loss'][-1]):.6f}; W rel err ours "
          f"{rel_err(model.W.weight.detach(), ref['W']):.3e} torch {rel_err(t32['W'], ref['W']):.3e}")
    assert abs(loss - loss_t) <= 1e-3 * max(1.0, abs(loss_t))
    pred = lambda Wm, bm: (Xd @ Wm.t() + bm).argmax(1)  # noqa: E731
    acc = float((pred(model.W.weight.detach(), model.W.bias.detach()) == yd).float().mean())
    acc_t = float((pred(t32["W"], t32["b"]) == yd).float().mean())
    assert acc == acc_t, (acc, acc_t)
    assert float(opt.state[model.W.weight]["step"]) == 100.0


def test_run_epochs_second_call_does_not_synchronise(monkeypatch):
    from sgc_amd.optim import Adam
    M, K, C = 60, 500, 3
    X, W, b, y = problem(M, K, C)
    model = sgc_pair(K, C, W, b)[0]
    Xd, yd = X.to(DEV), y.to(DEV)
    opt = Adam(model.parameters(), lr=0.2, weight_decay=WD)
    opt.run_epochs(model, Xd, yd, 2)  # the labels' one range check
    torch.cuda.synchronize()
    calls = {"sync": 0, "item": 0, "float": 0}

    def counted(key, fn):
        def w(*args, **kw):
            calls[key] += 1
            return fn(*args, **kw)
        return w
    monkeypatch.setattr(torch.cuda, "synchronize", counted("sync", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "__float__", counted("float", torch.Tensor.__float__))
    out = opt.run_epochs(model, Xd, yd, 5)
    monkeypatch.undo()
    assert calls == {"sync": 0, "item": 0, "float": 0}, calls
    assert out.dim() == 0 and float(opt.state[model.W.bias]["step"]) == 7.0


def test_step_run_epochs_step_equals_five_steps():
    """step(), run_epochs(3), step() leaves what five step()s leave, each
    within the bound against ref_train; a later call continues the state."""
    from sgc_amd.optim import Adam
    shape = (140, 1433, 7)
    (X, W, b, y), ref, t32 = references(*shape, epochs=5)
    Xd, yd = X.to(DEV), y.to(DEV)

    def manual(model, opt, n):
        for _ in range(n):
            model.train()
            opt.zero_grad()
            F.cross_entropy(model(Xd), yd).backward()
            opt.step()
    results = []
    for mixed in (True, False):
        model = sgc_pair(shape[1], shape[2], W, b)[0]
        opt = Adam(model.parameters(), lr=LR, weight_decay=WD)
        if mixed:
            manual(model, opt, 1)
            opt.run_epochs(model, Xd, yd, 3)
            manual(model, opt, 1)
        else:
            manual(model, opt, 5)
        st = opt.state
        assert float(st[model.W.weight]["step"]) == 5.0
        results.append(dict(W=model.W.weight.detach(), b=model.W.bias.detach(),
                            mW=st[model.W.weight]["exp_avg"], vW=st[model.W.weight]["exp_avg_sq"],
                            mb=st[model.W.bias]["exp_avg"], vb=st[model.W.bias]["exp_avg_sq"]))
    t = {k: t32[k] for k in results[0]}
    check_bound(errors(results[0], ref, t), "step, run_epochs(3), step")
    check_bound(errors(results[1], ref, t), "five step()s")


def test_run_epochs_fallbacks_and_labels():
    from sgc_amd.optim import Adam
    M, K, C = 37, 65, 17
    X, W, b, y = problem(M, K, C)
    Xd, yd = X.to(DEV), y.to(DEV)
    model = sgc_pair(K, C, W, b)[0]
    opt = Adam(model.parameters(), lr=LR, weight_decay=WD)
    bad = yd.clone()
    bad[5] = C
    with pytest.raises(IndexError):
        opt.run_epochs(model, Xd, bad, 1)
    assert len(opt.state) == 0  # nothing moved
    ignored = yd.clone()
    ignored[5] = -100
    out = opt.run_epochs(model, Xd, ignored, 2)  # the Python loop: -100 rows are left out
    assert out.dim() == 0 and model.W.weight.grad is not None
    assert float(opt.state[model.W.weight]["step"]) == 2.0
    out = opt.run_epochs(model, Xd.bfloat16(), yd, 1)  # 16-bit features: the Python loop too
    assert float(opt.state[model.W.weight]["step"]) == 3.0 and bool(torch.isfinite(out))
    assert opt.run_epochs(model, Xd, yd, 0) is None
