"""LBFGS.run_steps / sgc_train_lbfgs_f32 on the GPU.  The oracle is exact: the
stepwise device optimiser with the closure `sgc_cross_entropy(...).backward()`
runs the same sgc_linear_xent_f32 launches (grad_loss is 1.0, so p.grad holds
the kernel's bits) and the same iterate kernel, so the fused run must equal it
bit for bit -- W, b, the whole device state, every status and every loss."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_lbfgs_host import (STOP_GTD, STOP_LOSS_CHANGE, STOP_MAX_EVAL, STOP_MAX_ITER, STOP_OPT,
                             STOP_OPT_AT_ENTRY, STOP_STEP_SMALL, ref_step)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def problem(M, K, C, layout="contiguous", seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g) * scale
    y = torch.randint(0, C, (M,), generator=g)
    if layout == "strided":  # ldx > K
        X = torch.cat([X, torch.zeros(M, 5)], 1).to(DEV)[:, :K]
    elif layout == "offset":  # the base one float past an aligned address
        flat = torch.zeros(M * K + 1)
        flat[1:] = X.reshape(-1)
        X = flat.to(DEV)[1:].view(M, K)
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
    """The oracle: `steps` step() calls of the device optimiser with the fused
    loss closure.  -> (optimiser, statuses, losses)."""
    from sgc_amd.models import sgc_cross_entropy
    from sgc_amd.optim import LBFGS
    opt = LBFGS(model.parameters(), **opts)
    assert opt.device_path()

    def closure():
        opt.zero_grad()
        loss = sgc_cross_entropy(model, X, y)
        loss.backward()
        return loss
    statuses, losses = [], []
    for _ in range(steps):
        losses.append(opt.step(closure).detach())
        statuses.append(opt.last_status)
    return opt, statuses, torch.stack(losses), closure


def fused(model, X, y, steps, **opts):
    from sgc_amd.optim import LBFGS
    opt = LBFGS(model.parameters(), **opts)
    losses = opt.run_steps(model, X, y, steps)
    assert all(p.grad is None for p in model.parameters())
    return opt, opt.step_statuses, losses


def same_bits(a, b):
    """equal including NaN payload-free positions"""
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32
                                              else a, b.view(torch.int32)
                                              if b.dtype == torch.float32 else b)


def assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2):
    assert s1 == s2, (s1, s2)
    assert same_bits(l1, l2), (l1, l2)
    assert same_bits(m1.W.weight.detach(), m2.W.weight.detach())
    assert same_bits(m1.W.bias.detach(), m2.W.bias.detach())
    assert torch.equal(o1._dev_state, o2._dev_state)
    assert o1.last_status == o2.last_status
    a, b = o1.state[o1._params[0]], o2.state[o2._params[0]]
    assert (a["n_iter"], a["func_evals"]) == (b["n_iter"], b["func_evals"])


def compare(M, K, C, layout="contiguous", steps=2, scale=1.0, **opts):
    X, y = problem(M, K, C, layout, scale=scale)
    m1, m2 = models(K, C)
    o1, s1, l1, _ = stepwise(m1, X, y, steps, **opts)
    o2, s2, l2 = fused(m2, X, y, steps, **opts)
    torch.cuda.synchronize()
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2)
    return s2


SHAPES = [(1, 1, 1), (70, 33, 3), (257, 64, 7), (300, 602, 41), (300, 40, 48), (300, 40, 49),
          (40, 1023, 64), (3000, 602, 41)]


@pytest.mark.parametrize("M,K,C", SHAPES)
@pytest.mark.parametrize("layout", ["contiguous", "strided", "offset"])
def test_bit_equal_to_the_stepwise_run(M, K, C, layout):
    """Every load width (odd K: scalar; 64: 16 B; 602: 8 B), one and several
    row slabs, the column-block / slab boundary at 48 / 49 classes, n = 65,536
    exactly (the iterate kernel's largest size class), ldx > K and an odd base."""
    statuses = compare(M, K, C, layout, steps=2, max_iter=5 if M * K > 100000 else 4)
    assert all(s[3] >= 1 for s in statuses)


# SHAPES' classes give 1, 3 and 4 class tiles; these give 2, once per load width
# of the contiguous layout: scalar, 8 B, and 16 B with a ragged second row block.
NT2_SHAPES = [(70, 33, 17), (70, 34, 32), (130, 64, 20)]


@pytest.mark.parametrize("M,K,C", NT2_SHAPES)
@pytest.mark.parametrize("layout", ["contiguous", "strided", "offset"])
def test_bit_equal_with_two_class_tiles(M, K, C, layout):
    statuses = compare(M, K, C, layout, steps=2, max_iter=4)
    assert all(s[3] >= 1 for s in statuses)


@pytest.mark.parametrize("C", [3, 17, 41, 49])
def test_bit_equal_with_two_tile_buffers(C):
    """tile_buffers = 2 (the double-buffered LDS image of launch A), one class
    count per number of class tiles."""
    from sgc_amd import _lib
    lib = _lib.load()
    before = lib.sgc_get_tuning(b"tile_buffers")
    assert lib.sgc_set_tuning(b"tile_buffers", 2) == 0
    try:
        statuses = compare(130, 34, C, steps=2, max_iter=4)
    finally:
        restored = lib.sgc_set_tuning(b"tile_buffers", before)
    assert restored == 0
    assert all(s[3] >= 1 for s in statuses)


@pytest.mark.parametrize("value", [0, 1, 2, 3])
def test_bit_equal_under_each_backward_kernel(value):
    from sgc_amd import _lib
    lib = _lib.load()
    before = lib.sgc_get_tuning(b"backward_kernel")
    try:
        assert lib.sgc_set_tuning(b"backward_kernel", value) == 0
        compare(300, 602, 41, steps=2, max_iter=4)
    finally:
        assert lib.sgc_set_tuning(b"backward_kernel", before) == 0


# --- every stop reason ------------------------------------------------------------
# A small classifier problem (M=64, K=12, C=3); the option sets were chosen so
# that the fp64 restatement (ref_step) reaches each reason on the CPU.
STOP_CASES = {
    "opt_at_entry": (dict(tolerance_grad=10.0), STOP_OPT_AT_ENTRY),
    "max_iter": (dict(max_iter=4), STOP_MAX_ITER),  # (max_eval = 5: the iterations run out first)
    "max_eval": (dict(max_iter=10, max_eval=3), STOP_MAX_EVAL),
    "opt": (dict(max_iter=20, tolerance_grad=0.05), STOP_OPT),
    "gtd": (dict(tolerance_change=1e3), STOP_GTD),
    "step_small": (dict(lr=1e-6, tolerance_change=1e-5), STOP_STEP_SMALL),
    # lr = 0.2: in iteration 9 |dloss| = 0.0090 < 0.01 while max|t d| = 0.063 and |gtd| = 0.051;
    # every earlier iteration has |dloss| >= 0.0119
    "loss_change": (dict(lr=0.2, max_iter=20, tolerance_change=0.01), STOP_LOSS_CHANGE),
}


def stop_problem():
    X, y = problem(64, 12, 3, seed=5)
    (m,) = models(12, 3, n=1, seed=7)
    return X, y, m


def ref_run(X, y, model, opts):
    X64, yc = X.double().cpu(), y.cpu()
    C, K = model.W.weight.shape

    def f(x):
        return F.cross_entropy(X64 @ x[:C * K].view(C, K).t() + x[C * K:], yc)
    x = torch.cat([model.W.weight.detach().view(-1), model.W.bias.detach()]).double().cpu()
    st = {}
    reason = ref_step(f, x, st, **opts)
    return reason, st


@pytest.mark.parametrize("name", sorted(STOP_CASES))
def test_every_stop_reason(name):
    opts, want = STOP_CASES[name]
    X, y, m0 = stop_problem()
    reason, st = ref_run(X, y, m0, opts)
    assert reason == want, (name, reason)
    m1, m2 = models(12, 3, seed=7)
    o1, s1, l1, _ = stepwise(m1, X, y, 1, **opts)
    o2, s2, l2 = fused(m2, X, y, 1, **opts)
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2)
    n_iter, func_evals, _, _, stop, hist_len = s2[0]
    assert stop == want
    assert (n_iter, func_evals, hist_len) == (st["n_iter"], st["func_evals"],
                                              len(st.get("old_dirs") or []))


def test_stop_cases_cover_every_reason():
    assert {r for _, r in STOP_CASES.values()} == set(range(1, 8))


def test_stop_mid_run_and_next_steps_reset():
    """The second of three steps stops on its second closure (max_eval = 2):
    the skipped launches move nothing and the third step starts afresh."""
    statuses = compare(70, 33, 3, steps=3, max_iter=6, max_eval=2)
    assert [s[4] for s in statuses] == [STOP_MAX_EVAL] * 3 and statuses[1][3] == 2


def test_nan_stops_nothing_and_pushes_nothing():
    X, y = problem(70, 33, 3)
    X[5, 7] = float("inf")
    m1, m2 = models(33, 3)
    o1, s1, l1, _ = stepwise(m1, X, y, 2, max_iter=4)  # (max_eval = 5)
    o2, s2, l2 = fused(m2, X, y, 2, max_iter=4)
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, l2)
    assert bool(l2.isnan().all()) and s2[-1][5] == 0
    assert [s[2:5] for s in s2] == [(4, 4, STOP_MAX_ITER)] * 2  # every iteration taken


def test_fused_and_stepwise_steps_alternate():
    from sgc_amd.optim import LBFGS
    X, y = problem(257, 64, 7)
    m1, m2 = models(64, 7)
    o1, s1, l1, _ = stepwise(m1, X, y, 3, max_iter=4)
    from sgc_amd.models import sgc_cross_entropy
    o2 = LBFGS(m2.parameters(), max_iter=4)

    def closure():
        o2.zero_grad()
        loss = sgc_cross_entropy(m2, X, y)
        loss.backward()
        return loss
    s2, l2 = [], []
    l2.append(o2.run_steps(m2, X, y, 1)[0])
    s2.append(o2.last_status)
    l2.append(o2.step(closure).detach())
    s2.append(o2.last_status)
    l2.append(o2.run_steps(m2, X, y, 1)[0])
    s2.append(o2.last_status)
    assert_equal_runs(m1, o1, s1, l1, m2, o2, s2, torch.stack(l2))


def test_no_host_synchronisation(monkeypatch):
    import sgc_amd.optim as so
    X, y = problem(257, 64, 7)
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
    opt.run_steps(m, X, y, 2)
    monkeypatch.undo()
    assert calls == {"sync": 0, "item": 0, "float": 0, "read": 1, "step_read": 0}, calls
    assert all(p.grad is None for p in m.parameters())
    assert len(opt.step_statuses) == 2 and opt.step_statuses[-1] == opt.last_status


# --- fallbacks -----------------------------------------------------------------------

def literal_loop(opt, model, X, y, steps):
    def closure():
        opt.zero_grad()
        loss = F.cross_entropy(model(X), y)
        loss.backward()
        return loss
    losses, statuses = [], []
    for _ in range(steps):
        losses.append(opt.step(closure).detach())
        statuses.append(opt.last_status)
    return torch.stack(losses), statuses


@pytest.mark.parametrize("case", ["bf16", "ignored", "bias_first", "foreign"])
def test_fallbacks_run_the_literal_loop(case):
    from sgc_amd.optim import LBFGS
    X, y = problem(70, 33, 3)
    m1, m2 = models(33, 3)
    if case == "bf16":
        X = X.bfloat16()
    if case == "ignored":
        y[::4] = -100
    if case == "foreign":
        torch.manual_seed(3)
        m1 = torch.nn.Linear(33, 3).to(DEV)
        m2 = torch.nn.Linear(33, 3).to(DEV)
        m2.load_state_dict(m1.state_dict())

    def params(m):
        return [m.W.bias, m.W.weight] if case == "bias_first" else list(m.parameters())
    o1 = LBFGS(params(m1), max_iter=4)
    want, statuses = literal_loop(o1, m1, X, y, 2)
    o2 = LBFGS(params(m2), max_iter=4)
    got = o2.run_steps(m2, X, y, 2)
    assert same_bits(got, want)
    assert o2.step_statuses == statuses and o2.last_status == statuses[-1]
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert same_bits(p.detach(), q.detach())
    assert torch.equal(o1._dev_state, o2._dev_state)


def test_bad_label_raises_index_error():
    from sgc_amd.optim import LBFGS
    X, y = problem(70, 33, 3)
    (m,) = models(33, 3, n=1)
    y[3] = 3
    with pytest.raises(IndexError):
        LBFGS(m.parameters(), max_iter=4).run_steps(m, X, y, 1)


def test_classifier_end_to_end_like_torch():
    """Shape and bound of test_gpu_lbfgs.test_classifier_end_to_end_like_torch:
    X 3000x602, 41 classes, 2 steps."""
    from sgc_amd.optim import LBFGS
    torch.manual_seed(0)
    X = torch.randn(3000, 602, device=DEV)
    y = torch.randint(0, 41, (3000,), device=DEV)
    m1, m2 = models(602, 41, seed=0)
    ours = LBFGS(m1.parameters(), lr=1)
    ours.run_steps(m1, X, y, 2)
    theirs = torch.optim.LBFGS(m2.parameters(), lr=1)

    def closure():
        theirs.zero_grad()
        loss = F.cross_entropy(m2(X), y)
        loss.backward()
        return loss
    for _ in range(2):
        theirs.step(closure)
    losses = [F.cross_entropy(m(X), y).item() for m in (m1, m2)]
    a, b = ours.state[ours._params[0]], theirs.state[theirs._params[0]]
    print("fused lbfgs end to end: losses", losses, "n_iter/func_evals",
          (a["n_iter"], a["func_evals"]), (b["n_iter"], b["func_evals"]))
    assert (a["n_iter"], a["func_evals"]) == (b["n_iter"], b["func_evals"])
    assert abs(losses[0] - losses[1]) <= 1e-3 * max(1.0, abs(losses[1])), losses


# --- raw ABI ---------------------------------------------------------------------------

def test_raw_abi_null_traces_no_bias_and_zero_steps():
    from sgc_amd import _lib
    lib = _lib.load()
    M, K, C = 70, 33, 3
    X, y = problem(M, K, C)
    torch.manual_seed(2)
    W0 = torch.randn(C, K, device=DEV) * 0.1
    stream = _lib.stream_handle(DEV)
    n = C * K

    def new_state():
        nbytes = lib.sgc_lbfgs_workspace(n, 10)
        st = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(lib.sgc_lbfgs_init(_lib.ptr(st), nbytes, n, 10, stream), "init")
        return st
    ws_bytes = lib.sgc_train_lbfgs_workspace(M, K, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def run(W, st, steps, losses, table):
        _lib.check(lib.sgc_train_lbfgs_f32(_lib.ptr(X), K, _lib.ptr(W), None, _lib.ptr(y), M, K, C,
                                           _lib.ptr(st), steps, 1.0, 4, 5, 1e-7, 1e-9,
                                           _lib.ptr(losses), _lib.ptr(table), _lib.ptr(ws),
                                           ws_bytes, stream), "train_lbfgs_f32")
    Wa, Wb, sa, sb = W0.clone(), W0.clone(), new_state(), new_state()
    losses = torch.zeros(2, device=DEV)
    table = torch.zeros(12, dtype=torch.int64, device=DEV)
    run(Wa, sa, 2, losses, table)
    run(Wb, sb, 2, None, None)  # both traces NULL
    torch.cuda.synchronize()
    assert same_bits(Wa, Wb) and torch.equal(sa, sb) and not torch.equal(Wa, W0)
    out = (ctypes.c_int64 * 6)()
    _lib.check(lib.sgc_lbfgs_read_status(_lib.ptr(sa), out, stream), "status")
    assert table[6:].tolist() == list(out) and out[4] == STOP_MAX_ITER
    assert bool((losses > 0).all())
    keep_W, keep_s = Wa.clone(), sa.clone()
    run(Wa, sa, 0, None, None)  # steps == 0 touches nothing
    torch.cuda.synchronize()
    assert same_bits(Wa, keep_W) and torch.equal(sa, keep_s)
