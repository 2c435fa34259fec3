"""L-BFGS checks that need no GPU: the fp64 restatement of torch's step that the
GPU tests compare against (`ref_step`, validated here against
torch.optim.LBFGS itself), the CPU fallback of sgc_amd.optim.LBFGS, the
argument rejections of the C entry points and the new symbols."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

(STOP_NONE, STOP_OPT_AT_ENTRY, STOP_MAX_ITER, STOP_MAX_EVAL, STOP_OPT, STOP_GTD, STOP_STEP_SMALL,
 STOP_LOSS_CHANGE) = range(8)


def ref_step(f, x, st, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7,
             tolerance_change=1e-9, history_size=100, trace=None):
    """torch.optim.LBFGS.step (line_search_fn=None) restated on one flat
    vector: `f(x) -> scalar loss` is evaluated with autograd at the float64
    tensor `x`, which is updated in place; `st` is torch's state dict (carried
    between calls).  Returns the stop reason.  Every comparison appends
    (name, value, threshold) to `trace`."""
    if max_eval is None:
        max_eval = max_iter * 5 // 4

    def rec(name, value, thr):
        if trace is not None:
            trace.append((name, float(value), float(thr)))

    def evaluate():
        xx = x.detach().clone().requires_grad_(True)
        loss = f(xx)
        (g,) = torch.autograd.grad(loss, xx, allow_unused=True)
        return float(loss.detach()), (torch.zeros_like(x) if g is None else g.detach())

    st.setdefault("func_evals", 0)
    st.setdefault("n_iter", 0)
    loss, g = evaluate()
    current_evals = 1
    st["func_evals"] += 1
    rec("gmax", g.abs().max(), tolerance_grad)
    if g.abs().max() <= tolerance_grad:
        return STOP_OPT_AT_ENTRY
    d, t = st.get("d"), st.get("t")
    old_dirs, old_stps, ro = st.get("old_dirs"), st.get("old_stps"), st.get("ro")
    H_diag, prev_g, prev_loss = st.get("H_diag"), st.get("prev_flat_grad"), st.get("prev_loss")
    n_iter = 0
    reason = STOP_NONE
    while n_iter < max_iter:
        n_iter += 1
        st["n_iter"] += 1
        if st["n_iter"] == 1:
            d = g.neg()
            old_dirs, old_stps, ro = [], [], []
            H_diag = 1
        else:
            y = g.sub(prev_g)
            s = d.mul(t)
            ys = y.dot(s)
            rec("ys", ys, 1e-10)
            if ys > 1e-10:
                if len(old_dirs) == history_size:
                    old_dirs.pop(0)
                    old_stps.pop(0)
                    ro.pop(0)
                old_dirs.append(y)
                old_stps.append(s)
                ro.append(1.0 / ys)
                H_diag = ys / y.dot(y)
            num_old = len(old_dirs)
            al = [None] * history_size
            q = g.neg()
            for i in range(num_old - 1, -1, -1):
                al[i] = old_stps[i].dot(q) * ro[i]
                q.add_(old_dirs[i], alpha=-al[i])
            d = r = torch.mul(q, H_diag)
            for i in range(num_old):
                be_i = old_dirs[i].dot(r) * ro[i]
                r.add_(old_stps[i], alpha=al[i] - be_i)
        prev_g = g.clone()
        prev_loss = loss
        if st["n_iter"] == 1:
            t = min(1.0, 1.0 / g.abs().sum()) * lr
        else:
            t = lr
        gtd = g.dot(d)
        rec("gtd", gtd, -tolerance_change)
        if gtd > -tolerance_change:
            reason = STOP_GTD
            break
        x.add_(d, alpha=t)
        if n_iter != max_iter:
            loss, g = evaluate()
            current_evals += 1
            st["func_evals"] += 1
        if n_iter == max_iter:
            reason = STOP_MAX_ITER
            break
        if current_evals >= max_eval:
            reason = STOP_MAX_EVAL
            break
        rec("gmax", g.abs().max(), tolerance_grad)
        if g.abs().max() <= tolerance_grad:
            reason = STOP_OPT
            break
        rec("tdmax", d.mul(t).abs().max(), tolerance_change)
        if d.mul(t).abs().max() <= tolerance_change:
            reason = STOP_STEP_SMALL
            break
        rec("dloss", abs(loss - prev_loss), tolerance_change)
        if abs(loss - prev_loss) < tolerance_change:
            reason = STOP_LOSS_CHANGE
            break
    st.update(d=d, t=t, old_dirs=old_dirs, old_stps=old_stps, ro=ro, H_diag=H_diag,
              prev_flat_grad=prev_g, prev_loss=prev_loss)
    return reason


def assert_not_borderline(trace):
    """Every compared quantity is at least 1e-3 (relative) away from its
    threshold (a NaN never is borderline: all its comparisons are false)."""
    for name, v, thr in trace:
        if math.isnan(v):
            continue
        assert abs(v - thr) >= 1e-3 * max(abs(v), abs(thr)), (name, v, thr)


# --- the problems ---------------------------------------------------------------
# Each: shapes of the parameter tensors, x0(n) -> flat start (float64, values
# exact in float32), f(flat) -> loss (any dtype / device), optimiser options,
# number of step() calls, the stop reason of every step.

def _grid(n, lo, hi):
    """n values in [lo, hi], exact in float32 (multiples of 1/256)."""
    k = torch.arange(n, dtype=torch.float64)
    return lo + torch.floor(((k * 37) % 101) / 100.0 * (hi - lo) * 256) / 256


def quadratic(n):
    a, c = _grid(n, 1.0, 2.0), _grid(n, -1.0, 1.0)
    return lambda x: 0.5 * (a.to(x) * (x - c.to(x)) ** 2).sum()


def logistic(M=256, K=30, C=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g, dtype=torch.float64).float().double()
    y = torch.randint(0, C, (M,), generator=g)

    def f(x):
        W, b = x[:C * K].view(C, K), x[C * K:]
        return torch.nn.functional.cross_entropy(X.to(x) @ W.t() + b, y.to(x.device))
    return f, C * K + C


def _loss_change_f(x):
    w = torch.tensor([0.9, 0.05, 0.05, 0.05, 0.05], dtype=torch.float64)
    return (w.to(x) * x).sum()


def _nan_f(x):
    return (x * x).sum() * float("nan")


CASES = {
    # zero gradient at entry
    "opt_at_entry": dict(shapes=[(65,)], f=lambda x: (x * 0.0).sum(), opts={}, steps=1,
                         reasons=[STOP_OPT_AT_ENTRY]),
    "max_eval": dict(shapes=[(65,)], f=quadratic(65), opts=dict(max_iter=10, max_eval=3), steps=1,
                     reasons=[STOP_MAX_EVAL]),
    # isotropic quadratic, |g|_1 = 63/128 <= 1: t = 1 lands on the optimum
    "one_step_opt": dict(shapes=[(63,)],
                         f=lambda x: 0.5 * ((x - (1.0 / 128)) ** 2).sum(), opts={}, steps=1,
                         reasons=[STOP_OPT]),
    "gtd": dict(shapes=[(7, 9), (7,)], f=quadratic(70), opts=dict(tolerance_change=1e3), steps=1,
                reasons=[STOP_GTD]),
    # g = 1 at n = 4096: t = 1/4096, max|t d| = 2.4e-4 <= 1e-3
    "step_small": dict(shapes=[(4096,)], f=lambda x: x.sum(), opts=dict(tolerance_change=1e-3),
                       steps=1, reasons=[STOP_STEP_SMALL]),
    # linear objective: y = 0, ys = 0, nothing is pushed
    "linear_no_push": dict(shapes=[(5,), (1,), (1019,)],
                           f=lambda x: (_grid(1025, 0.5, 1.5).to(x) * x).sum(),
                           opts=dict(max_iter=4), steps=1, reasons=[STOP_MAX_ITER]),
    # g = (0.9, 0.05 x 4): |dloss| = 0.745 < 0.78 < max|t d| = 0.818, |gtd| = 0.82
    "loss_change": dict(shapes=[(5,)], f=_loss_change_f, opts=dict(tolerance_change=0.78),
                        steps=1, reasons=[STOP_LOSS_CHANGE]),
    "two_steps": dict(shapes=[(5, 30), (5,)], f=logistic()[0], opts=dict(max_iter=4), steps=2,
                      reasons=[STOP_MAX_ITER, STOP_MAX_ITER]),
    "ring_wraps": dict(shapes=[(155,)], f=logistic()[0], opts=dict(max_iter=8, max_eval=20,
                                                                   history_size=3),
                       steps=1, reasons=[STOP_MAX_ITER]),
    "nan_loss": dict(shapes=[(64,)], f=_nan_f, opts=dict(max_iter=3, max_eval=10), steps=1,
                     reasons=[STOP_MAX_ITER]),
}
for _n in (1, 63, 64, 65, 1023, 1025, 4097, 24723, 65536):
    CASES[f"quadratic_n{_n}"] = dict(shapes=[(_n,)], f=quadratic(_n),
                                     opts=dict(max_iter=3, max_eval=10, tolerance_grad=1e-4),
                                     steps=1,
                                     # (the secant step solves a 1-D quadratic exactly)
                                     reasons=[STOP_OPT if _n == 1 else STOP_MAX_ITER])


def case_numel(case):
    return sum(math.prod(s) for s in case["shapes"])


def case_x0(case):
    return _grid(case_numel(case), -0.5, 0.5) if case is not CASES["one_step_opt"] and \
        case is not CASES["loss_change"] else torch.zeros(case_numel(case), dtype=torch.float64)


def run_ref(case, trace=None):
    """(x, state, reasons) of `steps` ref_step calls from the case's start."""
    x, st, reasons = case_x0(case).clone(), {}, []
    for _ in range(case["steps"]):
        reasons.append(ref_step(case["f"], x, st, trace=trace, **case["opts"]))
    return x, st, reasons


def make_params(case, dtype, device):
    x0 = case_x0(case)
    ps, off = [], 0
    for s in case["shapes"]:
        k = math.prod(s)
        ps.append(x0[off:off + k].view(s).to(device=device, dtype=dtype).clone().requires_grad_(True))
        off += k
    return ps


def make_closure(case, opt, ps):
    def closure():
        opt.zero_grad()
        loss = case["f"](torch.cat([p.view(-1) for p in ps]))
        loss.backward()
        return loss
    return closure


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref_step_is_torch_lbfgs_in_float64(name):
    """The yardstick: ref_step reproduces torch.optim.LBFGS on CPU float64 bit
    for bit, stops for the reason the case is named for, and takes no
    borderline decision."""
    case = CASES[name]
    trace = []
    x, st, reasons = run_ref(case, trace)
    assert reasons == case["reasons"]
    assert_not_borderline(trace)
    ps = make_params(case, torch.float64, "cpu")
    opt = torch.optim.LBFGS(ps, **case["opts"])
    closure = make_closure(case, opt, ps)
    for _ in range(case["steps"]):
        opt.step(closure)
    flat = torch.cat([p.detach().view(-1) for p in ps])
    assert torch.equal(flat.nan_to_num(nan=1234.5), x.nan_to_num(nan=1234.5))
    tst = opt.state[ps[0]]
    assert (tst["n_iter"], tst["func_evals"]) == (st["n_iter"], st["func_evals"])
    assert len(tst.get("old_dirs") or []) == len(st.get("old_dirs") or [])


def test_every_stop_reason_is_covered():
    seen = {r for c in CASES.values() for r in c["reasons"]}
    assert seen == set(range(1, 8))


@pytest.mark.parametrize("name", ["two_steps", "quadratic_n1025", "gtd"])
def test_cpu_parameters_take_torch_step_bit_for_bit(name):
    from sgc_amd.optim import LBFGS
    case = CASES[name]
    out = []
    for cls in (torch.optim.LBFGS, LBFGS):
        ps = make_params(case, torch.float32, "cpu")
        opt = cls(ps, **case["opts"])
        closure = make_closure(case, opt, ps)
        for _ in range(2):
            opt.step(closure)
        out.append((torch.cat([p.detach().view(-1) for p in ps]), opt.state[ps[0]]["n_iter"],
                    opt.state[ps[0]]["func_evals"]))
        if cls is LBFGS:
            assert not opt.device_path()
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][1:] == out[1][1:]


def test_constructor_matches_torch():
    import inspect
    from sgc_amd.optim import LBFGS
    ours = list(inspect.signature(LBFGS.__init__).parameters)
    theirs = list(inspect.signature(torch.optim.LBFGS.__init__).parameters)
    assert ours == theirs + ["poll_every"]
    with pytest.raises(ValueError):
        LBFGS([torch.zeros(3, requires_grad=True)], poll_every=0)
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_optim",
                                                  os.path.join(ROOT, "dropin", "optim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.LBFGS is LBFGS


# --- C ABI ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from sgc_amd import build
    build.build(verbose=False)
    from sgc_amd import _lib
    return _lib.load()


def test_symbols_declared_and_bound():
    from sgc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sgc_lbfgs_workspace", "sgc_lbfgs_init", "sgc_lbfgs_begin_step",
                 "sgc_lbfgs_iterate_f32", "sgc_lbfgs_read_status"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    names = ["NONE", "OPT_AT_ENTRY", "MAX_ITER", "MAX_EVAL", "OPT", "GTD", "STEP_SMALL",
             "LOSS_CHANGE"]
    for value, nm in enumerate(names):
        assert re.search(r"SGC_LBFGS_STOP_%s = %d\b" % (nm, value), code), nm
    assert "#define SGC_ABI_VERSION 1" in hdr


def test_workspace_size_and_range(lib):
    ld = (24723 + 31) // 32 * 32
    assert lib.sgc_lbfgs_workspace(24723, 100) >= (2 * 100 + 2) * ld * 4 + 100 * 4 + 104
    assert lib.sgc_lbfgs_workspace(1, 1) > 0
    assert lib.sgc_lbfgs_workspace(65536, 1024) > 0
    for n, m, text in ((0, 10, b"n=0 < 1"), (65537, 10, b"n=65537 > 65536"),
                       (10, 0, b"history_size=0 < 1"), (10, 1025, b"history_size=1025 > 1024")):
        assert lib.sgc_lbfgs_workspace(n, m) == 0
        assert text in lib.sgc_last_error(), (n, m, lib.sgc_last_error())


def test_argument_rejections_before_any_device_call(lib):
    """Null device pointers throughout: every call stops at its argument
    checks with its code and text."""
    EINVAL, ERANGE, ENOMEM = 1, 2, 4
    fake = ctypes.c_void_p(256 * 4096)  # never dereferenced: the checks come first

    def err():
        return lib.sgc_last_error()
    assert lib.sgc_lbfgs_init(None, 1 << 20, 10, 5, None) == EINVAL and b"null state" in err()
    assert lib.sgc_lbfgs_init(fake, 1 << 20, 0, 5, None) == EINVAL and b"n=0 < 1" in err()
    assert lib.sgc_lbfgs_init(fake, 1 << 30, 65537, 5, None) == ERANGE and b"65537" in err()
    assert lib.sgc_lbfgs_init(fake, 1 << 20, 10, 0, None) == EINVAL and \
        b"history_size=0 < 1" in err()
    assert lib.sgc_lbfgs_init(fake, 1 << 20, 10, 1025, None) == ERANGE and b"1025" in err()
    assert lib.sgc_lbfgs_init(fake, 16, 10, 5, None) == ENOMEM and b"bytes" in err()
    assert lib.sgc_lbfgs_init(ctypes.c_void_p(256 * 4096 + 4), 1 << 20, 10, 5, None) == EINVAL \
        and b"aligned" in err()
    assert lib.sgc_lbfgs_begin_step(None, None) == EINVAL and b"null state" in err()
    out = (ctypes.c_int64 * 6)()
    assert lib.sgc_lbfgs_read_status(None, out, None) == EINVAL and b"null state" in err()
    assert lib.sgc_lbfgs_read_status(fake, None, None) == EINVAL and b"null out_host" in err()

    ptrs = (ctypes.c_void_p * 17)()
    numels = (ctypes.c_int64 * 17)(*([4] * 17))

    def iterate(state, nt, p=ptrs, g=ptrs, k=numels, max_iter=20):
        return lib.sgc_lbfgs_iterate_f32(state, nt, p, g, k, None, 1.0, max_iter, 25, 1e-7, 1e-9,
                                         None)
    assert iterate(None, 2) == EINVAL and b"null state" in err()
    for nt in (0, 17, -1):
        assert iterate(fake, nt) == EINVAL and b"outside 1..16" in err()
    assert iterate(fake, 2, p=None) == EINVAL and b"null pointer table" in err()
    assert iterate(fake, 2, g=None) == EINVAL and b"null pointer table" in err()
    assert iterate(fake, 2, k=None) == EINVAL and b"null pointer table" in err()
    assert iterate(fake, 2, max_iter=0) == EINVAL and b"max_iter" in err()
    neg = (ctypes.c_int64 * 2)(4, -1)
    assert iterate(fake, 2, k=neg) == EINVAL and b"numels[1]=-1" in err()
    big = (ctypes.c_int64 * 2)(65536, 1)
    assert iterate(fake, 2, k=big) == ERANGE and b"65536" in err()
    zero = (ctypes.c_int64 * 2)(0, 0)
    assert iterate(fake, 2, k=zero) == EINVAL and b"n=0 < 1" in err()
    # a state sgc_lbfgs_init never saw (the numels are checked against the n
    # it recorded; the sum test itself needs an initialised state: GPU suite)
    assert iterate(fake, 2) == EINVAL and b"not initialised" in err()
