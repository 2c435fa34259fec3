"""The wide L-BFGS iteration (csrc/lbfgs_wide.hip) on the GPU: one iteration
against the fp64 restatement with test_gpu_lbfgs.py's method and bound, whole
steps through the raw ABI against `ref_step`, the incrementally kept Gram block
against sgc_lbfgs_wide_sync_gram, stops and NaN, determinism, the narrow path
kept below the limit, sgc_train_lbfgs_wide_f32 against the stepwise wide path
and against fp64 torch.optim.LBFGS, textsgc.train_linear / eval_linear, and the
no-synchronisation-per-iteration property."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import test_gpu_lbfgs as narrow
from test_lbfgs_host import (STOP_GTD, STOP_MAX_EVAL, STOP_MAX_ITER, STOP_NONE, logistic,
                             quadratic, ref_step)
from test_lbfgs_wide_host import WIDE_CASES, documented_bytes, run_ref_wide, wide_x0

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, FILL = 5, -7.25


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import _lib
    return _lib.load()


def up(v, a):
    return (v + a - 1) // a * a


class State:
    """A wide device state and views of its documented blocks."""

    def __init__(self, lib, n, hs):
        from sgc_amd import _lib
        self.lib, self.n, self.hs = lib, n, hs
        nbytes = lib.sgc_lbfgs_wide_workspace(n, hs)
        assert nbytes == documented_bytes(n, hs)
        self.buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
        self.buf[nbytes:] = 0x5A  # guard past the state
        self.nbytes = nbytes
        self.stream = _lib.stream_handle(DEV)
        _lib.check(lib.sgc_lbfgs_wide_init(_lib.ptr(self.buf), nbytes, n, hs, self.stream), "init")
        torch.cuda.synchronize()
        ld = self.ld = up(n, 32)
        B = 2 * hs + 1
        off = 256
        self.ro = self.buf[off:off + hs * 4].view(torch.float32)
        off += up(hs * 4, 256)
        self.rows = self.buf[off:off + (4 + 2 * hs) * ld * 4].view(torch.float32).view(-1, ld)
        off += (4 + 2 * hs) * ld * 4 + up(B * 8, 256) + up((16 + 6 * hs) * 8, 256)
        self.G = self.buf[off:off + B * B * 8].view(torch.float64).view(B, B)
        self.ints = self.buf[:160].view(torch.int64)

    def ptr(self):
        from sgc_amd import _lib
        return _lib.ptr(self.buf)

    def state_bytes(self):
        return self.buf[:self.nbytes]

    def guard_ok(self):
        return bool((self.buf[self.nbytes:] == 0x5A).all())

    def begin(self):
        from sgc_amd import _lib
        _lib.check(self.lib.sgc_lbfgs_wide_begin_step(self.ptr(), self.stream), "begin")

    def iterate(self, ps, gs, loss, lr=1.0, max_iter=1000, max_eval=1000, tg=0.0, tc=0.0):
        from sgc_amd import _lib
        nt = len(ps)
        _lib.check(self.lib.sgc_lbfgs_wide_iterate_f32(
            self.ptr(), nt, (ctypes.c_void_p * nt)(*[t.data_ptr() for t in ps]),
            (ctypes.c_void_p * nt)(*[None if g is None else g.data_ptr() for g in gs]),
            (ctypes.c_int64 * nt)(*[t.numel() for t in ps]), _lib.ptr(loss), lr, max_iter,
            max_eval, tg, tc, self.stream), "iterate")

    def status(self):
        from sgc_amd import _lib
        out = (ctypes.c_int64 * 6)()
        _lib.check(self.lib.sgc_lbfgs_wide_read_status(self.ptr(), out, self.stream), "status")
        return tuple(out)

    def sync_gram(self):
        from sgc_amd import _lib
        _lib.check(self.lib.sgc_lbfgs_wide_sync_gram(self.ptr(), self.stream), "sync_gram")

    def clone(self):
        """A second registered state with this one's bytes."""
        other = State(self.lib, self.n, self.hs)
        other.buf[:self.nbytes].copy_(self.buf[:self.nbytes])
        return other

    def load_torch(self, st, head):
        """torch's state `st` (fp32-rounded) into the documented layout."""
        n, hs, ints = self.n, self.hs, self.ints
        m = len(st["old_dirs"])
        assert ints[7:10].tolist() == [n, hs, self.ld]
        ints[0], ints[1], ints[5], ints[6] = st["n_iter"], st["func_evals"], m, head % hs
        self.buf[80:96].view(torch.float64)[1] = st["prev_loss"]
        self.buf[96:104].view(torch.float32).copy_(
            torch.tensor([float(st["H_diag"]), float(st["t"])]))
        self.rows[0, :n] = st["d"].float().to(DEV)
        self.rows[1, :n] = st["prev_flat_grad"].float().to(DEV)
        for i in range(m):
            slot = (head + i) % hs
            self.ro[slot] = float(st["ro"][i])
            self.rows[2 + slot, :n] = st["old_stps"][i].float().to(DEV)
            self.rows[2 + hs + slot, :n] = st["old_dirs"][i].float().to(DEV)
        self.sync_gram()


def guarded(flat, shapes):
    """Separate allocations per tensor, each with GUARD fill elements behind."""
    bufs, views, off = [], [], 0
    for s in shapes:
        k = math.prod(s)
        buf = torch.full((k + GUARD,), FILL, dtype=torch.float32, device=DEV)
        buf[:k] = flat[off:off + k]
        bufs.append(buf)
        views.append(buf[:k])
        off += k
    return bufs, views


def guards_ok(bufs):
    return all(bool((b[-GUARD:] == FILL).all()) for b in bufs)


# --- one iteration -----------------------------------------------------------------

def one_iteration(lib, f, n, shapes, j, hs, head=0, lr=1.0):
    """test_gpu_lbfgs.one_iteration on the wide state."""
    narrow.HISTORY[0] = hs
    lr = float(torch.tensor(lr).float())
    x = (torch.arange(1, n + 1, dtype=torch.float64) * 0.37).sin() * 0.25 + 0.25
    st = {}
    ref_step(f, x, st, lr=lr, max_iter=j, max_eval=10 ** 6, tolerance_grad=0.0,
             tolerance_change=0.0, history_size=hs)
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
        return narrow.iteration_math(c(p32), c(g32), c(f32["d"]), c(f32["t"]), c(f32["prev_g"]),
                                     [c(s) for s in f32["S"]], [c(y) for y in f32["Y"]],
                                     [c(r) for r in f32["ro"]], c(f32["H_diag"]), lr)
    d64, p64 = math_in(torch.float64, "cpu")
    dt, pt = math_in(torch.float32, DEV)

    state = State(lib, n, hs)
    state.load_torch(st, head)
    pbufs, ps = guarded(p32.to(DEV), shapes)
    gbufs, gs = guarded(g32.to(DEV), shapes)
    lbuf = torch.full((1 + GUARD,), FILL, device=DEV)
    lbuf[0] = loss32
    state.begin()
    state.iterate(ps, gs, lbuf[:1], lr=lr)
    out = state.status()
    assert list(out) == [j + 1, st["func_evals"] + 1, 1, 1, STOP_NONE, min(hs, m + 1)]
    d_ours = state.rows[0, :n]
    p_ours = torch.cat([t.view(-1) for t in ps])
    assert bool((state.rows[:, n:] == 0).all())  # the pad columns stay zero
    assert guards_ok(pbufs) and guards_ok(gbufs) and guards_ok([lbuf]) and state.guard_ok()
    assert torch.equal(torch.cat(gs), g32.to(DEV))  # the gradient is only read
    return {"d": (narrow.rel_err(d_ours, d64), narrow.rel_err(dt, d64)),
            "p": (narrow.rel_err(p_ours, p64), narrow.rel_err(pt, p64))}, m


@pytest.mark.parametrize("j,hs,head,m_want", [(1, 100, 0, 0), (2, 100, 0, 1), (4, 100, 0, 3),
                                               (41, 100, 0, 40), (8, 3, 1, 3)])
def test_one_iteration_logistic(lib, j, hs, head, m_want):
    f, n = logistic()
    errs, m = one_iteration(lib, f, n, [(5, 30), (5,)], j, hs, head, lr=0.1)
    assert m == m_want
    narrow.check_bound(errs, f"wide logistic m={m} history_size={hs}")


@pytest.mark.parametrize("n", [1, 65, 4097, 65536, 65537, 69333])
def test_one_iteration_sizes(lib, n):
    """Three tensors at odd offsets (one at n = 1), around the narrow limit."""
    shapes = [(n,)] if n < 7 else [(5,), (1,), (n - 6,)]
    j = 1 if n == 1 else 3
    errs, m = one_iteration(lib, quadratic(n), n, shapes, j, 100)
    assert m == j - 1
    narrow.check_bound(errs, f"wide quadratic n={n}")


def test_one_iteration_20ng_size(lib):
    """n = 20 x 61,603: tiles of 4096 floats, 301 workgroups."""
    n = 1232060
    errs, m = one_iteration(lib, quadratic(n), n, [(5,), (1,), (n - 6,)], 3, 4)
    assert m == 2
    narrow.check_bound(errs, f"wide quadratic n={n}")


# --- whole steps through the raw ABI --------------------------------------------------

def run_raw(lib, name, watch=None, extra_after_stop=0):
    """The case's steps: per step the reset, then max_iter times [closure on
    the device in fp32, iterate].  -> (flat, statuses, state, params)."""
    case = WIDE_CASES[name]
    opts = dict(lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
                history_size=100)
    opts.update(case["opts"])
    if opts["max_eval"] is None:
        opts["max_eval"] = opts["max_iter"] * 5 // 4
    x0 = wide_x0(name).float().to(DEV)
    n = x0.numel()
    shapes = case["shapes"]
    _, ps = guarded(x0, shapes)
    state = State(lib, n, opts["history_size"])
    statuses = []
    for _ in range(case["steps"]):
        state.begin()
        for it in range(opts["max_iter"] + extra_after_stop):
            flat = torch.cat([p.view(-1) for p in ps]).requires_grad_(True)
            loss = case["f"](flat)
            (g,) = torch.autograd.grad(loss, flat, allow_unused=True)
            g = torch.zeros_like(flat) if g is None else g
            _, gs = guarded(g, shapes)
            state.iterate(ps, gs, loss.detach().float().reshape(1), opts["lr"], opts["max_iter"],
                          opts["max_eval"], opts["tolerance_grad"], opts["tolerance_change"])
            if watch is not None:
                torch.cuda.synchronize()
                watch(state, ps, it)
        statuses.append(state.status())
    torch.cuda.synchronize()
    return torch.cat([p.view(-1) for p in ps]), statuses, state, ps


DEVICE_REASONS = {}  # case -> the stop reason of each step as the device returned it


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_ref_wide(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(WIDE_CASES))
def test_whole_steps_match_ref_step(lib, refs, name):
    """Statuses equal ref_step's; the parameters are held to what
    test_gpu_lbfgs.test_control_flow_matches_ref_step holds the narrow path to
    (finite, untouched on a GTD stop, NaN where torch's are), and their
    distance to the fp64 run is printed."""
    case = WIDE_CASES[name]
    x64, st, reasons = refs(name)
    flat, statuses, state, _ = run_raw(lib, name)
    DEVICE_REASONS[name] = [s[4] for s in statuses]
    assert [s[4] for s in statuses] == reasons
    n_iter, func_evals, _, _, _, hist_len = statuses[-1]
    assert (n_iter, func_evals, hist_len) == (st["n_iter"], st["func_evals"],
                                              len(st.get("old_dirs") or []))
    if reasons[-1] == STOP_GTD and case["steps"] == 1:
        assert torch.equal(flat.cpu(), wide_x0(name).float())
    if name == "nan_loss":
        assert bool(flat.isnan().all()) and hist_len == 0
    else:
        assert bool(torch.isfinite(flat).all())
        print(f"wide whole steps {name}: rel. distance to fp64 "
              f"{narrow.rel_err(flat, x64) if float(x64.norm()) > 0 else 0.0:.3e}")
    if name == "linear_no_push":
        assert hist_len == 0
    if name == "two_steps":
        assert hist_len == 7 and statuses[0][5] == 3
    assert bool((state.rows[:, state.n:] == 0).all()) or name == "nan_loss"
    assert state.guard_ok()


def test_every_stop_reason_is_reached(lib):
    """Over what the device returned: the runs of
    test_whole_steps_match_ref_step, and a run here of any case that test has
    not run in this session."""
    for name in WIDE_CASES:
        if name not in DEVICE_REASONS:
            DEVICE_REASONS[name] = [s[4] for s in run_raw(lib, name)[1]]
    assert sorted(DEVICE_REASONS) == sorted(WIDE_CASES)
    assert {r for rs in DEVICE_REASONS.values() for r in rs} == set(range(1, 8))


def test_numels_must_sum_to_the_states_n(lib):
    state = State(lib, 70000, 4)
    ptrs = (ctypes.c_void_p * 2)()
    rc = lib.sgc_lbfgs_wide_iterate_f32(state.ptr(), 2, ptrs, ptrs,
                                        (ctypes.c_int64 * 2)(40000, 29999), None, 1.0, 20, 25,
                                        1e-7, 1e-9, None)
    assert rc == 1 and b"numels sum to 69999" in lib.sgc_last_error()
    torch.cuda.synchronize()


def test_either_init_replaces_the_registry_entry(lib):
    """One address initialised by one engine, then by the other: the registry
    keeps the last init only, so the first engine's calls are refused at their
    argument checks (nothing is launched) and the second engine's run."""
    from sgc_amd import _lib
    n, hs = 40, 3
    nbytes = lib.sgc_lbfgs_wide_workspace(n, hs)
    assert nbytes >= lib.sgc_lbfgs_workspace(n, hs) > 0
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    stream = _lib.stream_handle(DEV)
    p = torch.ones(n, device=DEV)
    g = torch.full((n,), 0.5, device=DEV)
    loss = torch.ones(1, device=DEV)
    args = (_lib.ptr(buf), 1, (ctypes.c_void_p * 1)(p.data_ptr()),
            (ctypes.c_void_p * 1)(g.data_ptr()), (ctypes.c_int64 * 1)(n), _lib.ptr(loss), 1.0, 20,
            25, 1e-7, 1e-9, stream)

    def refused(rc, init):
        return rc == 1 and b"not initialised by " + init in lib.sgc_last_error()
    _lib.check(lib.sgc_lbfgs_init(_lib.ptr(buf), nbytes, n, hs, stream), "init")
    _lib.check(lib.sgc_lbfgs_wide_init(_lib.ptr(buf), nbytes, n, hs, stream), "wide_init")
    assert refused(lib.sgc_lbfgs_iterate_f32(*args), b"sgc_lbfgs_init")
    assert lib.sgc_lbfgs_wide_iterate_f32(*args) == 0
    _lib.check(lib.sgc_lbfgs_init(_lib.ptr(buf), nbytes, n, hs, stream), "init")
    assert refused(lib.sgc_lbfgs_wide_iterate_f32(*args), b"sgc_lbfgs_wide_init")
    assert refused(lib.sgc_lbfgs_wide_sync_gram(_lib.ptr(buf), stream), b"sgc_lbfgs_wide_init")
    assert refused(lib.sgc_lbfgs_wide_l2_f32(_lib.ptr(buf), _lib.ptr(p), _lib.ptr(g), n, 1e-3,
                                             _lib.ptr(loss), stream), b"sgc_lbfgs_wide_init")
    assert lib.sgc_lbfgs_iterate_f32(*args) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(p).all()


# --- the Gram block ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["reject_full_ring", "full_ring", "two_steps"])
def test_incremental_gram_block_is_the_synced_block(lib, name):
    """After every device iteration -- across the ring wrap and, in
    reject_full_ring, a pair rejected with the ring full -- the block kept
    incrementally equals, bit for bit, the block sync_gram computes from the
    rows of a copy of the state."""
    seen = {"rejected_full": 0, "pushed": 0, "checked": 0}
    prev = {"n_iter": 0, "hist": 0}

    def watch(state, ps, it):
        n_iter, hist = int(state.ints[0]), int(state.ints[5])
        if n_iter == prev["n_iter"]:
            return
        pushed = int(state.ints[15])
        if pushed:
            seen["pushed"] += 1
        elif n_iter > 1 and prev["hist"] == state.hs:
            seen["rejected_full"] += 1
        prev.update(n_iter=n_iter, hist=hist)
        copy = state.clone()
        copy.sync_gram()
        torch.cuda.synchronize()
        assert torch.equal(state.G.view(torch.int64), copy.G.view(torch.int64)), (name, n_iter)
        seen["checked"] += 1
    run_raw(lib, name, watch=watch)
    assert seen["checked"] >= 8 and seen["pushed"] >= 4
    if name == "reject_full_ring":
        assert seen["rejected_full"] >= 1


# --- stops and NaN ----------------------------------------------------------------------

@pytest.mark.parametrize("name,reason", [("max_eval", STOP_MAX_EVAL), ("gtd", STOP_GTD),
                                         ("linear_no_push", STOP_MAX_ITER)])
def test_stopped_step_changes_nothing(lib, name, reason):
    """Once the step has stopped, further launches (iterations and the L2
    step) change no byte of the state, the parameters or the gradient."""
    from sgc_amd import _lib
    snap = {}

    def watch(state, ps, it):
        stop = int(state.ints[4])
        if stop and "state" not in snap:
            snap.update(state=state.state_bytes().clone(), ps=[p.clone() for p in ps], at=it)
        elif stop:
            w, gw = ps[-1], torch.ones_like(ps[-1])
            loss = torch.ones(1, device=DEV)
            _lib.check(lib.sgc_lbfgs_wide_l2_f32(state.ptr(), _lib.ptr(w), _lib.ptr(gw),
                                                 w.numel(), 0.5, _lib.ptr(loss), state.stream),
                       "l2")
            torch.cuda.synchronize()
            assert float(loss) == 1.0 and bool((gw == 1).all())
            assert torch.equal(state.state_bytes(), snap["state"])
            assert all(torch.equal(a, b) for a, b in zip(ps, snap["ps"]))
            snap["later"] = snap.get("later", 0) + 1
    _, statuses, _, _ = run_raw(lib, name, watch=watch, extra_after_stop=3)
    assert statuses[-1][4] == reason and snap["later"] >= 3


def test_nan_loss_with_a_finite_gradient_stops_nothing(lib):
    """All of torch's tests are false on NaN: with a NaN loss and finite
    gradients the run is the finite run."""
    n = 70000
    a = torch.linspace(1.0, 2.0, n, device=DEV)
    out = []
    for nan in (False, True):
        p = torch.zeros(n, device=DEV)
        state = State(lib, n, 5)
        state.begin()
        for _ in range(6):
            g = a * (p - 1.0)
            loss = (0.5 * (a * (p - 1.0) ** 2).sum()).reshape(1)
            state.iterate([p], [g], loss * float("nan") if nan else loss, 1.0, 6, 100, 1e-7, 1e-9)
        out.append((p, state.status()))
    assert out[0][1] == out[1][1] == (6, 6, 6, 6, STOP_MAX_ITER, 5)
    assert torch.equal(out[0][0], out[1][0])


def test_two_runs_are_bitwise_equal(lib):
    runs = [run_raw(lib, "reject_full_ring") for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2].state_bytes(), runs[1][2].state_bytes())


# --- sgc_amd.optim.LBFGS(wide=True) -----------------------------------------------------

def classifier_problem(M, K, C, scale, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(M, K, generator=g) * scale).to(DEV)
    y = torch.randint(0, C, (M,), generator=g).to(DEV)
    torch.manual_seed(1)
    W0 = torch.randn(C, K) * 0.01
    return X, y, W0


def test_narrow_path_kept_below_the_limit():
    """n = 24,723 (Reddit): wide=True runs the narrow kernel, the same bits."""
    from sgc_amd.models import SGC
    from sgc_amd.optim import LBFGS
    X, y, _ = classifier_problem(300, 602, 41, 1.0)
    torch.manual_seed(2)
    ms = [SGC(602, 41).to(DEV) for _ in range(2)]
    ms[1].load_state_dict(ms[0].state_dict())
    opts = []
    for m, kw in zip(ms, ({}, {"wide": True})):
        opt = LBFGS(m.parameters(), max_iter=5, **kw)

        def closure():
            opt.zero_grad()
            loss = F.cross_entropy(m(X), y)
            loss.backward()
            return loss
        opt.step(closure)
        opts.append(opt)
    torch.cuda.synchronize()
    assert opts[1].wide and not opts[1]._dev_wide
    assert torch.equal(ms[0].W.weight, ms[1].W.weight) and torch.equal(ms[0].W.bias, ms[1].W.bias)
    assert torch.equal(opts[0]._dev_state, opts[1]._dev_state)
    assert opts[0].last_status == opts[1].last_status


def test_above_the_limit_wide_takes_the_device_path():
    from sgc_amd.optim import LBFGS
    big = torch.zeros(65537, device=DEV, requires_grad=True)
    a = torch.linspace(1.0, 2.0, 65537, device=DEV)
    assert not LBFGS([big]).device_path()  # today's class: torch's own step there
    opt = LBFGS([big], max_iter=4, wide=True)
    assert opt.device_path()

    def closure():
        opt.zero_grad()
        loss = 0.5 * (a * (big - 1.0) ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)
    assert opt._dev_wide and opt.last_status[:4] == (4, 4, 4, 4)
    assert opt.last_status[4] == STOP_MAX_ITER and opt.state[big]["n_iter"] == 4
    twin = torch.zeros(65537, device=DEV, requires_grad=True)
    ref = torch.optim.LBFGS([twin], max_iter=4)

    def closure2():
        ref.zero_grad()
        loss = 0.5 * (a * (twin - 1.0) ** 2).sum()
        loss.backward()
        return loss
    ref.step(closure2)
    assert float((big - twin).abs().max()) <= 1e-4


def test_no_host_synchronisation_per_iteration(monkeypatch):
    import sgc_amd.optim as so
    n = 70001
    a = torch.linspace(1.0, 2.0, n, device=DEV)
    p = torch.zeros(n, device=DEV, requires_grad=True)
    opt = so.LBFGS([p], max_iter=6, wide=True)

    def closure():
        opt.zero_grad()
        loss = 0.5 * (a * (p - 1.0) ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)  # builds the state
    torch.cuda.synchronize()
    assert opt._dev_wide
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
    assert opt.last_status[3] >= 2


# --- fused training ---------------------------------------------------------------------

def make_model(K, C, bias, W0):
    from sgc_amd.textsgc import SGC
    m = SGC(K, C, bias=bias).to(DEV)
    with torch.no_grad():
        m.W.weight.copy_(W0)
        if bias:
            m.W.bias.zero_()
    return m


def stepwise_wide(lib, model, X, y, steps, l2, max_iter, history_size):
    """The oracle of the fused call: the same steps driven closure by closure
    through sgc_linear_xent_f32, sgc_lbfgs_wide_l2_f32 and
    sgc_lbfgs_wide_iterate_f32."""
    from sgc_amd import _lib
    W, b = model.W.weight.data, None if model.W.bias is None else model.W.bias.data
    M, K = X.shape
    C = W.shape[0]
    n = W.numel() + (0 if b is None else C)
    state = State(lib, n, history_size)
    wsb = lib.sgc_linear_xent_workspace(M, K, C)
    ws = torch.empty(max(1, wsb), dtype=torch.uint8, device=DEV)
    dW, db = torch.empty_like(W), torch.empty(C, device=DEV)
    loss = torch.empty(1, device=DEV)
    max_eval = max_iter * 5 // 4
    losses, statuses, first = [], [], {}
    ps = [W] if b is None else [W, b]
    gs = [dW] if b is None else [dW, db]
    for s in range(steps):
        state.begin()
        for it in range(max_iter):
            _lib.check(lib.sgc_linear_xent_f32(
                _lib.ptr(X), X.stride(0), _lib.ptr(W), _lib.ptr(b), _lib.ptr(y), M, K, C,
                _lib.ptr(loss), _lib.ptr(dW), None if b is None else _lib.ptr(db), None, 0,
                _lib.ptr(ws), ws.numel(), state.stream), "linear_xent")
            if s == 0 and it == 0:
                first.update(loss=loss.clone(), dW=dW.clone(), db=db.clone())
            stopped = int(state.ints[4]) != 0
            _lib.check(lib.sgc_lbfgs_wide_l2_f32(state.ptr(), _lib.ptr(W), _lib.ptr(dW),
                                                 W.numel(), l2, _lib.ptr(loss), state.stream), "l2")
            if it == 0:
                losses.append(loss.clone())
            if stopped:
                break  # (the stepwise closure is not behind the stop word)
            state.iterate(ps, gs, loss, 1.0, max_iter, max_eval, 1e-7, 1e-9)
        statuses.append(state.status())
    torch.cuda.synchronize()
    return state, statuses, torch.cat(losses), first


def torch_fp64(X, y, W0, bias, l2, steps, max_iter, history_size):
    """torch.optim.LBFGS in fp64 on the reference closure (the L2 term on W)."""
    X64, yc = X.double().cpu(), y.cpu()
    W = W0.double().clone().requires_grad_(True)
    ps = [W]
    if bias:
        b = torch.zeros(W.shape[0], dtype=torch.float64, requires_grad=True)
        ps.append(b)
    opt = torch.optim.LBFGS(ps, max_iter=max_iter, history_size=history_size)

    def closure():
        opt.zero_grad()
        out = X64 @ W.t() + (b if bias else 0.0)
        loss = F.nll_loss(F.log_softmax(out, dim=1), yc) + 0.5 * l2 * (W ** 2).sum()
        loss.backward()
        return loss
    for _ in range(steps):
        opt.step(closure)
    st = opt.state[W]
    return st["n_iter"], st["func_evals"], float(closure().detach())


FUSED = [(37, 2100, 33, True, 0.1, 100), (37, 2100, 33, False, 0.1, 100),
         (129, 1100, 61, True, 0.1, 100), (48, 64, 17, True, 1.0, 100),
         (37, 2100, 33, False, 0.1, 3)]


@pytest.mark.parametrize("l2", [0.0, 5e-4])
@pytest.mark.parametrize("M,K,C,bias,scale,hs", FUSED)
def test_fused_training(lib, M, K, C, bias, scale, hs, l2):
    """sgc_train_lbfgs_wide_f32 (through run_steps) = the stepwise wide path
    bit for bit; its first closure with l2 = 0 = sgc_linear_xent_f32; the run
    = fp64 torch.optim.LBFGS on the reference closure in n_iter / func_evals
    and, to test_gpu_lbfgs_train.py's tolerance, in the final loss."""
    from sgc_amd.optim import LBFGS
    X, y, W0 = classifier_problem(M, K, C, scale)
    steps, max_iter = 3, 20
    m1, m2 = make_model(K, C, bias, W0), make_model(K, C, bias, W0)
    state, statuses, losses, first = stepwise_wide(lib, m1, X, y, steps, l2, max_iter, hs)
    opt = LBFGS(m2.parameters(), max_iter=max_iter, history_size=hs, wide=True)
    got = opt.run_steps(m2, X, y, steps, l2=l2)
    torch.cuda.synchronize()
    assert opt._dev_wide and all(p.grad is None for p in m2.parameters())
    assert opt.step_statuses == statuses
    assert torch.equal(got.view(torch.int32), losses.view(torch.int32))
    assert torch.equal(m1.W.weight.view(torch.int32), m2.W.weight.view(torch.int32))
    if bias:
        assert torch.equal(m1.W.bias.view(torch.int32), m2.W.bias.view(torch.int32))
    assert torch.equal(state.state_bytes(), opt._dev_state[:state.nbytes])
    if l2 == 0.0:
        assert torch.equal(got[:1].view(torch.int32), first["loss"].view(torch.int32))
    n_iter, func_evals, ref_loss = torch_fp64(X, y, W0, bias, l2, steps, max_iter, hs)
    with torch.no_grad():
        ours = float(F.cross_entropy(F.linear(X, m2.W.weight, m2.W.bias), y) +
                     0.5 * l2 * (m2.W.weight ** 2).sum())
    print(f"fused wide {M}x{K}x{C} bias={bias} l2={l2} hs={hs}: loss {ours:.6e} fp64 torch "
          f"{ref_loss:.6e}; n_iter/func_evals {statuses[-1][:2]} torch {(n_iter, func_evals)}")
    assert statuses[-1][:2] == (n_iter, func_evals)
    assert abs(ours - ref_loss) <= 1e-3 * max(1.0, abs(ref_loss))


def test_shape_the_closure_refuses_runs_the_literal_loop(monkeypatch):
    """run_steps probes the fused call's argument checks (steps = 0) and takes
    the literal loop on SGC_ERANGE.  No testable shape is past the closure's
    31-bit offsets, so the probe's verdict is forced here: the literal loop
    with the L2 term must then do what the fused call does."""
    import sgc_amd.optim as so
    X, y, W0 = classifier_problem(48, 64, 17, 1.0)
    m1, m2 = make_model(64, 17, True, W0), make_model(64, 17, True, W0)
    fused = so.LBFGS(m1.parameters(), max_iter=4, wide=True)
    l1 = fused.run_steps(m1, X, y, 2, l2=5e-4)
    monkeypatch.setattr(so, "_SGC_ERANGE", 0)  # the probe's SGC_OK now reads as a refusal
    literal = so.LBFGS(m2.parameters(), max_iter=4, wide=True)
    l2 = literal.run_steps(m2, X, y, 2, l2=5e-4)
    monkeypatch.undo()
    assert all(p.grad is not None for p in m2.parameters())  # closures ran through autograd
    assert [s[:5] for s in literal.step_statuses] == [s[:5] for s in fused.step_statuses]
    # the two closures are different fp32 kernels: test_gpu_lbfgs_train.py's
    # tolerance for such a pair of runs
    finals = [float(F.cross_entropy(F.linear(X, m.W.weight, m.W.bias), y)) for m in (m1, m2)]
    print("literal loop after a refused probe: first losses", l1.tolist(), l2.tolist(),
          "final", finals)
    assert float((l1 - l2).abs().max()) <= 1e-3 * max(1.0, float(l1.abs().max()))
    assert abs(finals[0] - finals[1]) <= 1e-3 * max(1.0, abs(finals[1]))


def test_fused_first_closure_is_linear_xent(lib):
    """With l2 = 0 the first closure's loss and gradient are
    sgc_linear_xent_f32's bits: one step of max_iter = 1 at lr = 0 leaves the
    gradient in prev_g and W where it was."""
    from sgc_amd.optim import LBFGS
    M, K, C = 37, 2100, 33
    X, y, W0 = classifier_problem(M, K, C, 0.1)
    m1, m2 = make_model(K, C, True, W0), make_model(K, C, True, W0)
    _, _, losses, first = stepwise_wide(lib, m1, X, y, 1, 0.0, 1, 4)
    opt = LBFGS(m2.parameters(), lr=0.0, max_iter=1, history_size=4, wide=True)
    got = opt.run_steps(m2, X, y, 1)
    torch.cuda.synchronize()
    n = C * K + C
    off = 256 + up(4 * 4, 256)
    prev_g = opt._dev_state[off:off + 4 * up(n, 32) * 6].view(torch.float32).view(6, -1)[1, :n]
    want = torch.cat([first["dW"].view(-1), first["db"]])
    assert torch.equal(prev_g.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.view(torch.int32), first["loss"].view(torch.int32))


# --- textsgc ----------------------------------------------------------------------------

def reference_train_eval(W0, feats, labels, weight_decay, epochs, binary):
    """The reference's train_linear / eval_linear in torch ops (nn.Linear,
    torch.optim.LBFGS), on the device."""
    lin = torch.nn.Linear(W0.shape[1], W0.shape[0], bias=False).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W0)
    act = torch.sigmoid if binary else (lambda o: F.log_softmax(o, dim=1))
    crit = F.binary_cross_entropy if binary else F.nll_loss
    opt = torch.optim.LBFGS(lin.parameters())
    for _ in range(epochs):
        def closure():
            opt.zero_grad()
            out = lin(feats["train"]).squeeze()
            loss = crit(act(out), labels["train"]) + 0.5 * weight_decay * (lin.weight ** 2).sum()
            loss.backward()
            return loss
        opt.step(closure)
    with torch.no_grad():
        out = lin(feats["val"]).squeeze()
        loss = crit(act(out), labels["val"]).item()
        pred = act(out).gt(0.5).float() if binary else out.max(1)[1]
        acc = torch.eq(pred, labels["val"]).long().sum().item() / pred.size(0)
    return acc, loss


@pytest.mark.parametrize("binary", [False, True])
def test_textsgc_train_and_eval_linear(binary):
    """300 documents, K = 2,500 and 30 classes (n = 75,000: the wide path);
    binary: one sigmoid output."""
    from sgc_amd import textsgc
    K, C = 2500, (1 if binary else 30)
    g = torch.Generator().manual_seed(5)
    proto = torch.rand(30, K, generator=g)
    feats, labels = {}, {}
    for split, m in (("train", 200), ("val", 100)):
        cls = torch.randint(0, 30, (m,), generator=g)
        x = (0.6 * proto[cls] + 0.4 * torch.rand(m, K, generator=g)) / 8.0
        feats[split] = x.to(DEV)
        labels[split] = (cls.ge(15).float() if binary else cls).to(DEV)
    torch.manual_seed(7)
    model = textsgc.SGC(K, C).to(DEV)
    W0 = model.W.weight.detach().clone()
    want_acc, want_loss = reference_train_eval(W0, feats, labels, 5e-4, 3, binary)
    acc, out, seconds = textsgc.train_linear(model, feats, labels, 5e-4, epochs=3, binary=binary)
    res = textsgc.eval_linear(model, feats["val"], labels["val"], binary)
    print(f"textsgc binary={binary}: acc {acc} loss {res['loss']:.6f}; torch ops acc {want_acc} "
          f"loss {want_loss:.6f}")
    assert out is model and seconds > 0 and res["accuracy"] == acc
    assert abs(acc - want_acc) <= 1e-3 * max(1.0, want_acc)
    assert abs(res["loss"] - want_loss) <= 1e-3 * max(1.0, abs(want_loss))
