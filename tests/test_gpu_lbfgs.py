"""sgc_amd.optim.LBFGS on the GPU: one device iteration against the fp64
restatement and against torch's fp32 arithmetic, the control flow of whole
steps against `ref_step` (tests/test_lbfgs_host.py, validated there against
torch.optim.LBFGS), determinism, the end-to-end classifier run and the
no-synchronisation-per-iteration property."""
import ctypes
import math

import pytest
import torch

from test_lbfgs_host import (CASES, STOP_GTD, STOP_NONE, case_x0, logistic, make_closure, make_params,
                             quadratic, ref_step, run_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 2.0 ** -22  # four fp32 epsilons


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import _lib
    return _lib.load()


# --- one iteration -----------------------------------------------------------------

def split(flat, shapes):
    """Separate allocations per tensor (later ones start at odd offsets of the
    flat vector)."""
    out, off = [], 0
    for s in shapes:
        k = math.prod(s)
        out.append(flat[off:off + k].clone().view(s))
        off += k
    return out


def iteration_math(p, g, d, t, prev_g, S, Y, ro, H_diag, lr):
    """What torch.optim.LBFGS does in an iteration after the first, with
    torch ops in the dtype / on the device of its inputs.  -> (d, p)."""
    S, Y, ro = list(S), list(Y), list(ro)
    y = g.sub(prev_g)
    s = d.mul(t)
    ys = y.dot(s)
    if ys > 1e-10:
        if len(S) == HISTORY[0]:
            S.pop(0), Y.pop(0), ro.pop(0)
        Y.append(y), S.append(s), ro.append(1.0 / ys)
        H_diag = ys / y.dot(y)
    al = [None] * len(S)
    q = g.neg()
    for i in range(len(S) - 1, -1, -1):
        al[i] = S[i].dot(q) * ro[i]
        q.add_(Y[i], alpha=-al[i])
    r = torch.mul(q, H_diag)
    for i in range(len(S)):
        be_i = Y[i].dot(r) * ro[i]
        r.add_(S[i], alpha=al[i] - be_i)
    return r, p.add(r, alpha=lr)


HISTORY = [100]  # history_size iteration_math drops pairs at


def load_state(lib, n, hs, st, head):
    """A device state holding torch's state `st` (fp32-rounded): the layout
    include/sgc_amd.h documents."""
    from sgc_amd import _lib
    nbytes = lib.sgc_lbfgs_workspace(n, hs)
    state = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.sgc_lbfgs_init(_lib.ptr(state), nbytes, n, hs, _lib.stream_handle(DEV)), "init")
    torch.cuda.synchronize()
    ld = (n + 31) // 32 * 32
    m = len(st["old_dirs"])
    ints = state[:80].view(torch.int64)
    assert ints[7:10].tolist() == [n, hs, ld]
    ints[0], ints[1], ints[5], ints[6] = st["n_iter"], st["func_evals"], m, head % hs
    state[80:96].view(torch.float64)[1] = st["prev_loss"]
    state[96:104].view(torch.float32).copy_(torch.tensor([float(st["H_diag"]), float(st["t"])]))
    off = 256
    ro_bytes = (hs * 4 + 255) // 256 * 256
    ro = state[off:off + hs * 4].view(torch.float32)
    rows = state[off + ro_bytes:].view(torch.float32)[:(2 + 2 * hs) * ld].view(2 + 2 * hs, ld)
    rows[0, :n] = st["d"].float().to(DEV)
    rows[1, :n] = st["prev_flat_grad"].float().to(DEV)
    for i in range(m):
        slot = (head + i) % hs
        ro[slot] = float(st["ro"][i])
        rows[2 + slot, :n] = st["old_stps"][i].float().to(DEV)
        rows[2 + hs + slot, :n] = st["old_dirs"][i].float().to(DEV)
    return state, rows


def rel_err(x, x64):
    return float((x.double().cpu() - x64).norm() / x64.norm())


def one_iteration(lib, f, n, shapes, j, hs, head=0, lr=1.0):
    """State after j fp64 iterations, rounded to fp32; then one device
    iteration vs the fp64 restatement and vs torch's fp32 ops on the same
    inputs.  -> {"d": (e_ours, e_torch32), "p": (...)}, m."""
    from sgc_amd import _lib
    HISTORY[0] = hs
    lr = float(torch.tensor(lr).float())  # as the device rounds it
    x = (torch.arange(1, n + 1, dtype=torch.float64) * 0.37).sin() * 0.25 + 0.25
    st = {}
    ref_step(f, x, st, lr=lr, max_iter=j, max_eval=10 ** 6, tolerance_grad=0.0, tolerance_change=0.0,
             history_size=hs)
    assert st["n_iter"] == j
    m = len(st["old_dirs"])
    p32 = x.float()
    xx = p32.double().requires_grad_(True)
    loss = f(xx)
    (g,) = torch.autograd.grad(loss, xx)
    g32, loss32 = g.float(), loss.detach().float()
    f32 = dict(d=st["d"].float(), t=torch.tensor(float(st["t"])).float(),
               prev_g=st["prev_flat_grad"].float(), S=[s.float() for s in st["old_stps"]],
               Y=[y.float() for y in st["old_dirs"]],
               ro=[torch.as_tensor(r).float() for r in st["ro"]],
               H_diag=torch.as_tensor(st["H_diag"]).float())

    def math_in(dtype, device):
        c = lambda v: v.to(device=device, dtype=dtype)  # noqa: E731
        return iteration_math(c(p32), c(g32), c(f32["d"]), c(f32["t"]), c(f32["prev_g"]),
                              [c(s) for s in f32["S"]], [c(y) for y in f32["Y"]],
                              [c(r) for r in f32["ro"]], c(f32["H_diag"]), lr)
    d64, p64 = math_in(torch.float64, "cpu")
    dt, pt = math_in(torch.float32, DEV)

    state, rows = load_state(lib, n, hs, st, head)
    ps, gs = split(p32.to(DEV), shapes), split(g32.to(DEV), shapes)
    nt = len(ps)
    loss_dev = loss32.to(DEV)
    stream = _lib.stream_handle(DEV)
    _lib.check(lib.sgc_lbfgs_begin_step(_lib.ptr(state), stream), "begin")
    _lib.check(lib.sgc_lbfgs_iterate_f32(
        _lib.ptr(state), nt, (ctypes.c_void_p * nt)(*[t.data_ptr() for t in ps]),
        (ctypes.c_void_p * nt)(*[t.data_ptr() for t in gs]),
        (ctypes.c_int64 * nt)(*[t.numel() for t in ps]), _lib.ptr(loss_dev), lr, 1000, 1000,
        0.0, 0.0, stream), "iterate")
    out = (ctypes.c_int64 * 6)()
    _lib.check(lib.sgc_lbfgs_read_status(_lib.ptr(state), out, stream), "status")
    m_new = min(hs, m + 1)
    assert list(out) == [j + 1, st["func_evals"] + 1, 1, 1, STOP_NONE, m_new]
    d_ours = rows[0, :n]
    p_ours = torch.cat([t.view(-1) for t in ps])
    assert bool((rows[:, n:] == 0).all())  # the pad columns stay zero
    return {"d": (rel_err(d_ours, d64), rel_err(dt, d64)),
            "p": (rel_err(p_ours, p64), rel_err(pt, p64))}, m


def check_bound(errs, what):
    for k, (ours, t32) in errs.items():
        print(f"lbfgs one iteration {what}: {k}: e(ours)={ours:.3e} e(torch fp32)={t32:.3e}")
    for k, (ours, t32) in errs.items():
        assert ours <= 2 * t32 + FLOOR, (what, k, ours, t32)


@pytest.mark.parametrize("j,hs,head,m_want", [(1, 100, 0, 0), (2, 100, 0, 1), (4, 100, 0, 3),
                                               (41, 100, 0, 40), (8, 3, 1, 3)])
def test_one_iteration_logistic(lib, j, hs, head, m_want):
    """m = 0, 1, 3, 40 pairs and the wrapped ring (history_size=3 after 8
    iterations), logistic regression M=256 K=30 C=5, as [5x30, 5]; lr = 0.1,
    at which 41 iterations still make progress and push 40 pairs."""
    f, n = logistic()
    errs, m = one_iteration(lib, f, n, [(5, 30), (5,)], j, hs, head, lr=0.1)
    assert m == m_want
    check_bound(errs, f"logistic m={m} history_size={hs}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 4097, 24723, 65536])
def test_one_iteration_sizes(lib, n):
    """Every size class of the kernel (1, 2, 4, 8, 16 chunks per thread) and
    the sizes around a wave, the workgroup and a chunk, with two pairs (none at n = 1)."""
    shapes = [(n,)] if n < 1025 else [(5,), (1,), (n - 6,)]
    j = 1 if n == 1 else 3  # (the secant step solves n = 1 exactly: the device takes it)
    errs, m = one_iteration(lib, quadratic(n), n, shapes, j, 100)
    assert m == j - 1
    check_bound(errs, f"quadratic n={n}")


# --- whole steps ---------------------------------------------------------------------

def run_device(case, poll_every=None, float_loss=False):
    from sgc_amd.optim import LBFGS
    ps = make_params(case, torch.float32, DEV)
    opt = LBFGS(ps, poll_every=poll_every, **case["opts"])
    assert opt.device_path()
    inner = make_closure(case, opt, ps)
    closure = (lambda: float(inner().detach())) if float_loss else inner
    statuses = []
    for _ in range(case["steps"]):
        opt.step(closure)
        statuses.append(opt.last_status)
    torch.cuda.synchronize()
    return torch.cat([p.detach().view(-1) for p in ps]), statuses, opt


@pytest.fixture(scope="module")
def refs():
    """ref_step's result per case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_ref(CASES[name])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(CASES))
def test_control_flow_matches_ref_step(refs, name):
    case = CASES[name]
    x64, st, reasons = refs(name)
    flat, statuses, opt = run_device(case)
    assert [s[4] for s in statuses] == reasons
    n_iter, func_evals, _, _, _, hist_len = statuses[-1]
    assert (n_iter, func_evals, hist_len) == (st["n_iter"], st["func_evals"],
                                              len(st.get("old_dirs") or []))
    tstate = opt.state[opt._params[0]]
    assert (tstate["n_iter"], tstate["func_evals"]) == (st["n_iter"], st["func_evals"])
    if reasons[-1] == STOP_GTD and case["steps"] == 1:  # the parameters are untouched
        assert torch.equal(flat.cpu(), case_x0(case).float())
    if name == "nan_loss":
        assert bool(flat.isnan().all()) and hist_len == 0
    elif name == "linear_no_push":
        assert hist_len == 0
    elif name == "two_steps":
        assert hist_len == 7 and statuses[0][5] == 3  # the second step continues the history
    if name != "nan_loss":
        assert bool(torch.isfinite(flat).all())


def test_numels_must_sum_to_the_states_n(lib):
    from sgc_amd import _lib
    nbytes = lib.sgc_lbfgs_workspace(10, 4)
    state = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.sgc_lbfgs_init(_lib.ptr(state), nbytes, 10, 4, _lib.stream_handle(DEV)), "init")
    ptrs = (ctypes.c_void_p * 2)()
    rc = lib.sgc_lbfgs_iterate_f32(_lib.ptr(state), 2, ptrs, ptrs, (ctypes.c_int64 * 2)(4, 5), None,
                                   1.0, 20, 25, 1e-7, 1e-9, None)
    assert rc == 1 and b"numels sum to 9" in lib.sgc_last_error()
    torch.cuda.synchronize()


def test_fallbacks_and_changed_options():
    from sgc_amd.optim import LBFGS
    big = torch.zeros(65537, device=DEV, requires_grad=True)
    opt = LBFGS([big], max_iter=4)
    assert not opt.device_path()

    def closure():
        opt.zero_grad()
        loss = ((big - 1.0) ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)
    assert opt._dev_state is None and opt.last_status is None  # torch's own step ran
    assert opt.state[big]["n_iter"] >= 1 and float(big.detach().abs().max()) > 0
    wolfe = LBFGS([torch.zeros(8, device=DEV, requires_grad=True)], line_search_fn="strong_wolfe")
    assert not wolfe.device_path()
    case = CASES["two_steps"]
    ps = make_params(case, torch.float32, DEV)
    opt = LBFGS(ps, max_iter=2)
    c = make_closure(case, opt, ps)
    opt.step(c)
    opt.param_groups[0]["history_size"] = 7
    with pytest.raises(ValueError):
        opt.step(c)


def test_deterministic_and_poll_every_changes_nothing():
    case = CASES["max_eval"]  # stops early: the polled run leaves the loop
    runs = [run_device(CASES["two_steps"]) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][2]._dev_state, runs[1][2]._dev_state)
    assert runs[0][1] == runs[1][1]
    for c in (case, CASES["two_steps"]):
        a, b, fl = run_device(c), run_device(c, poll_every=1), run_device(c, float_loss=True)
        for other in (b, fl):
            assert torch.equal(a[0], other[0])
            assert a[1] == other[1]
            assert torch.equal(a[2]._dev_state, other[2]._dev_state)


def test_classifier_end_to_end_like_torch():
    """Shape and bound of test_fused_loss_trains_like_torch: X 3000x602, 41
    classes, 2 steps, the SGC model and the unchanged closure."""
    from sgc_amd.models import SGC
    from sgc_amd.optim import LBFGS
    torch.manual_seed(0)
    X = torch.randn(3000, 602, device=DEV)
    y = torch.randint(0, 41, (3000,), device=DEV)
    m1 = SGC(602, 41).to(DEV)
    m2 = SGC(602, 41).to(DEV)
    m2.load_state_dict(m1.state_dict())
    losses, counts = [], []
    for m, cls in ((m1, LBFGS), (m2, torch.optim.LBFGS)):
        opt = cls(m.parameters(), lr=1)

        def closure():
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(m(X), y)
            loss.backward()
            return loss
        for _ in range(2):
            opt.step(closure)
        losses.append(torch.nn.functional.cross_entropy(m(X), y).item())
        st = opt.state[opt._params[0]]
        counts.append((st["n_iter"], st["func_evals"]))
    print("lbfgs end to end: losses", losses, "n_iter/func_evals", counts)
    assert m1.W.weight.numel() + m1.W.bias.numel() == 24723
    assert abs(losses[0] - losses[1]) <= 1e-3 * max(1.0, abs(losses[1])), losses
    assert counts[0] == counts[1]


def test_no_host_synchronisation_per_iteration(monkeypatch):
    import sgc_amd.optim as so
    n = 1025
    a = torch.linspace(1.0, 2.0, n, device=DEV)
    p = torch.zeros(n, device=DEV, requires_grad=True)
    opt = so.LBFGS([p], max_iter=6)

    def closure():
        opt.zero_grad()
        loss = 0.5 * (a * (p - 1.0) ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)  # builds the state
    torch.cuda.synchronize()
    calls = {"sync": 0, "item": 0, "float": 0, "read": 0}

    def counted(key, fn):
        def w(*args, **kw):
            calls[key] += 1
            return fn(*args, **kw)
        return w
    monkeypatch.setattr(torch.cuda, "synchronize", counted("sync", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "__float__", counted("float", torch.Tensor.__float__))
    monkeypatch.setattr(so, "_read_status", counted("read", so._read_status))
    opt.step(closure)
    monkeypatch.undo()
    assert calls == {"sync": 0, "item": 0, "float": 0, "read": 1}, calls
    assert opt.last_status[3] >= 2  # several closures consumed, one read-back
