"""Adam checks that need no GPU: the fp64 restatements the GPU tests compare
against (tests/adam_ref.py, validated here against torch.optim.Adam itself),
the CPU fallbacks of sgc_amd.optim.Adam, the argument rejections of the C entry
points, the new symbols, and that the GPU one-step test's inputs and bound
tell every mutant of the restatement apart."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adam_ref import (FLOOR, LR, MUTANTS, ONE_STEP_CASES, adam_math, one_step_case,
                      one_step_errors, ref_adam_step, ref_train)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITATION_SHAPES = ((140, 1433, 7), (120, 3703, 6), (60, 500, 3))


def max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# --- the restatements against torch ---------------------------------------------------

@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_ref_adam_step_is_torch_adam_in_float64(wd):
    """Two param groups (their own lr and weight decay), a parameter whose
    grad stays None (skipped: no state), 5 steps."""
    gen = torch.Generator().manual_seed(3)
    shapes = [(7, 33), (7,), (5,), (4, 3)]
    ps = [torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in shapes]
    opt = torch.optim.Adam([{"params": ps[:3]}, {"params": ps[3:], "lr": 0.01, "weight_decay": 0.1}],
                           lr=0.2, weight_decay=wd)
    groups = [(0, 3, 0.2, wd), (3, 4, 0.01, 0.1)]
    P = [p.detach().clone() for p in ps]
    Ms, Vs = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    worst = 0.0
    for step in range(1, 6):
        grads = [None if i == 2 else 0.5 ** step * torch.randn(s, generator=gen, dtype=torch.float64)
                 for i, s in enumerate(shapes)]
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
        opt.step()
        for lo, hi, lr, w in groups:
            P[lo:hi], Ms[lo:hi], Vs[lo:hi] = ref_adam_step(P[lo:hi], grads[lo:hi], Ms[lo:hi],
                                                            Vs[lo:hi], step, lr, w)
        for i, p in enumerate(ps):
            worst = max(worst, max_rel(P[i], p.detach()))
            if i != 2:
                worst = max(worst, max_rel(Ms[i], opt.state[p]["exp_avg"]),
                            max_rel(Vs[i], opt.state[p]["exp_avg_sq"]))
    print(f"ref_adam_step vs torch.optim.Adam fp64, wd={wd}: max rel {worst:.3e}")
    assert worst <= 1e-14
    assert len(opt.state[ps[2]]) == 0 and torch.equal(P[2], ps[2].detach())


def small_problem(M=37, K=65, C=5, seed=0, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=gen, dtype=torch.float64)
    y = torch.randint(0, C, (M,), generator=gen)
    W = (torch.rand(C, K, generator=gen, dtype=torch.float64) * 2 - 1) / K ** 0.5
    b = (torch.rand(C, generator=gen, dtype=torch.float64) * 2 - 1) / K ** 0.5
    return X.to(dtype), W.to(dtype), b.to(dtype), y


@pytest.mark.parametrize("bias", [True, False])
def test_ref_train_is_the_autograd_loop_in_float64(bias):
    X, W0, b0, y = small_problem()
    W = W0.clone().requires_grad_(True)
    b = b0.clone().requires_grad_(True) if bias else None
    opt = torch.optim.Adam([W] + ([b] if bias else []), lr=0.2, weight_decay=5e-4)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = F.cross_entropy(F.linear(X, W, b), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    r = ref_train(X, W0, b0 if bias else None, y, 5, 0.2, 5e-4)
    worst = max(max_rel(r["W"], W.detach()), max_rel(r["loss"], torch.stack(losses)),
                max_rel(r["vW"], opt.state[W]["exp_avg_sq"]),
                max_rel(r["mW"], opt.state[W]["exp_avg"]))
    if bias:
        worst = max(worst, max_rel(r["b"], b.detach()), max_rel(r["mb"], opt.state[b]["exp_avg"]))
    print(f"ref_train vs autograd + torch.optim.Adam fp64: max rel {worst:.3e}")
    assert worst <= 1e-14


def test_mutants_are_told_apart_by_the_gpu_tests_inputs_and_bound():
    """Each mutant of the restatement misses the GPU one-step test's bound
    (2 x torch's fp32 error + FLOOR, the fp32 error taken as the worst over
    the cases measured here on the CPU) on at least one of that test's cases."""
    def as_dtype(dtype, mutant=None):
        def run(p, g, m, v, step, wd):
            return adam_math(p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype), step, LR, wd,
                             mutant=mutant)
        return run

    def numpy_mutant(mutant):
        def run(p, g, m, v, step, wd):
            out = adam_math(*(t.double().numpy() for t in (p, g, m, v)), step, LR, wd, mutant=mutant)
            return tuple(torch.from_numpy(np.asarray(o)) for o in out)
        return run
    t32 = {k: 0.0 for k in "pmv"}
    for case in ONE_STEP_CASES:
        for k, e in one_step_errors(case, as_dtype(torch.float32)).items():
            t32[k] = max(t32[k], e)
    print("worst torch fp32 (CPU) one-step errors:", t32)
    assert all(e < 1e-5 for e in t32.values())
    for mutant in MUTANTS:
        caught = []
        for case in ONE_STEP_CASES:
            for k, e in one_step_errors(case, numpy_mutant(mutant)).items():
                if not e <= 2 * t32[k] + FLOOR:  # (a NaN error is a miss too)
                    caught.append((case, k, e))
        print(f"mutant {mutant}: caught by {len(caught)} (case, output) pairs, e.g. {caught[:1]}")
        assert caught, mutant
    # the unmutated numpy restatement passes every case
    for case in ONE_STEP_CASES:
        assert all(e <= FLOOR for e in one_step_errors(case, numpy_mutant(None)).values())


# --- the Python class on the CPU ----------------------------------------------------------

def test_constructor_matches_torch():
    from sgc_amd.optim import Adam
    assert inspect.signature(Adam.__init__) == inspect.signature(torch.optim.Adam.__init__)
    assert issubclass(Adam, torch.optim.Adam)


def test_dropin_exports_adam():
    from sgc_amd.optim import Adam
    spec = importlib.util.spec_from_file_location("dropin_optim_adam",
                                                  os.path.join(ROOT, "dropin", "optim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.Adam is Adam and "Adam" in mod.__all__


def test_cpu_step_is_torch_adam_bit_for_bit():
    from sgc_amd.optim import Adam
    X, W0, b0, y = small_problem(dtype=torch.float32)
    runs = []
    for cls in (Adam, torch.optim.Adam):
        W, b = W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        opt = cls([W, b], lr=0.2, weight_decay=5e-4)
        for _ in range(4):
            opt.zero_grad()
            F.cross_entropy(F.linear(X, W, b), y).backward()
            opt.step()

        def closure():
            opt.zero_grad()
            loss = F.cross_entropy(F.linear(X, W, b), y)
            loss.backward()
            return loss
        loss = opt.step(closure)
        runs.append((W.detach(), b.detach(), opt.state[W]["exp_avg"], opt.state[W]["exp_avg_sq"],
                     opt.state[b]["step"], loss.detach()))
    for a, t in zip(*runs):
        assert torch.equal(a, t)


@pytest.mark.parametrize("trace", [False, True])
def test_cpu_run_epochs_is_torch_adam_bit_for_bit(trace):
    from sgc_amd.models import SGC
    from sgc_amd.optim import Adam
    X, W0, b0, y = small_problem(dtype=torch.float32)
    models = [SGC(X.shape[1], 5), SGC(X.shape[1], 5)]
    models[1].load_state_dict(models[0].state_dict())
    ours = Adam(models[0].parameters(), lr=0.2, weight_decay=5e-4)
    got = ours.run_epochs(models[0], X, y, 6, loss_trace=trace)
    theirs = torch.optim.Adam(models[1].parameters(), lr=0.2, weight_decay=5e-4)
    losses = []
    for _ in range(6):
        models[1].train()
        theirs.zero_grad()
        loss = F.cross_entropy(models[1](X), y)
        loss.backward()
        theirs.step()
        losses.append(loss.detach())
    assert torch.equal(got, torch.stack(losses) if trace else losses[-1])
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(ours.state[p]["exp_avg_sq"], theirs.state[q]["exp_avg_sq"])
        assert float(ours.state[p]["step"]) == 6.0
    before = [p.detach().clone() for p in models[0].parameters()]
    assert ours.run_epochs(models[0], X, y, 0) is None
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, models[0].parameters()))
    with pytest.raises(IndexError):
        bad = y.clone()
        bad[3] = 5
        ours.run_epochs(models[0], X, bad, 1)


def test_state_dict_round_trip():
    from sgc_amd.optim import Adam
    X, W0, b0, y = small_problem(dtype=torch.float32)

    def make():
        W, b = W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        return W, b, Adam([W, b], lr=0.2, weight_decay=5e-4)

    def steps(W, b, opt, n):
        for _ in range(n):
            opt.zero_grad()
            F.cross_entropy(F.linear(X, W, b), y).backward()
            opt.step()
    W1, b1, o1 = make()
    steps(W1, b1, o1, 5)
    W2, b2, o2 = make()
    steps(W2, b2, o2, 2)
    W3, b3, o3 = make()
    with torch.no_grad():
        W3.copy_(W2)
        b3.copy_(b2)
    o3.load_state_dict(o2.state_dict())
    assert set(o3.state[W3]) == {"step", "exp_avg", "exp_avg_sq"}
    steps(W3, b3, o3, 3)
    assert torch.equal(W3.detach(), W1.detach()) and torch.equal(b3.detach(), b1.detach())
    assert float(o3.state[W3]["step"]) == 5.0


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
    for name in ("sgc_adam_step_f32", "sgc_train_adam_workspace", "sgc_train_adam_f32"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert "#define SGC_ABI_VERSION 1" in hdr
    for text in ("g' = g + wd * p", "m  = m + (g' - m) * (1 - b1)", "\"adam_kernel\"", "313"):
        assert text in hdr, text


def test_workspace_sizes(lib):
    for M, K, C in CITATION_SHAPES:
        assert lib.sgc_train_adam_workspace(M, K, C) >= (K + 63) // 64 * M * 16 * 4
    for M, K, C in ((0, 10, 3), (10, 0, 3), (10, 10, 0)):
        assert lib.sgc_train_adam_workspace(M, K, C) == 0
    assert lib.sgc_get_tuning(b"adam_small_max_rows") == 313
    assert lib.sgc_get_tuning(b"adam_kernel") == 0
    assert lib.sgc_set_tuning(b"adam_kernel", 3) == 1 and b"adam_kernel" in lib.sgc_last_error()
    assert lib.sgc_get_tuning(b"adam_kernel") == 0


def test_argument_rejections_before_any_device_call(lib):
    """Null or fake device pointers throughout: every call stops at its
    argument checks with its code and text."""
    EINVAL, ENOMEM = 1, 4
    fake = ctypes.c_void_p(256 * 4096)  # never dereferenced: the checks come first

    def err():
        return lib.sgc_last_error()

    def tables(n):
        return (ctypes.c_void_p * max(n, 1))(*[fake.value] * max(n, 1)), \
            (ctypes.c_int64 * max(n, 1))(*[8] * max(n, 1))

    def step(n, step=1, tabs=True):
        t, numels = tables(n)
        a = (t, t, t, t, numels) if tabs else (None, None, None, None, None)
        return lib.sgc_adam_step_f32(n, *a, step, 0.2, 0.9, 0.999, 1e-8, 0.0, None)
    assert step(0) == EINVAL and b"n_tensors=0 outside 1..16" in err()
    assert step(17) == EINVAL and b"n_tensors=17 outside 1..16" in err()
    assert step(2, step=0) == EINVAL and b"step=0 < 1" in err()
    assert step(2, tabs=False) == EINVAL and b"null pointer table" in err()
    t, numels = tables(2)
    numels[1] = -1
    assert lib.sgc_adam_step_f32(2, t, t, t, t, numels, 1, 0.2, 0.9, 0.999, 1e-8, 0.0, None) == \
        EINVAL and b"numels[1]=-1" in err()
    nulls = (ctypes.c_void_p * 2)(fake.value, None)
    numels[1] = 8
    assert lib.sgc_adam_step_f32(2, nulls, t, t, t, numels, 1, 0.2, 0.9, 0.999, 1e-8, 0.0,
                                 None) == EINVAL and b"null parameter or moment 1" in err()

    def train(M=140, K=1433, C=7, ldx=None, b=fake, mb=fake, vb=fake, step0=0, epochs=3, ws=fake,
              ws_bytes=1 << 30, X=fake):
        return lib.sgc_train_adam_f32(X, K if ldx is None else ldx, fake, b, fake, M, K, C, fake,
                                      fake, mb, vb, step0, epochs, 0.2, 0.9, 0.999, 1e-8, 5e-4,
                                      None, ws, ws_bytes, None)
    assert train(epochs=-1) == EINVAL and b"epochs=-1 < 0" in err()
    assert train(C=0) == EINVAL and b"C=0" in err()
    assert train(C=65) == EINVAL and b"C=65" in err()
    assert train(M=0) == EINVAL and b"M=0" in err()
    assert train(ldx=1432) == EINVAL and b"ldx=1432" in err()
    assert train(step0=-1) == EINVAL and b"step0=-1 < 0" in err()
    assert train(b=None) == EINVAL and b"NULL together" in err()
    assert train(b=None, mb=None) == EINVAL and b"NULL together" in err()
    assert train(mb=None) == EINVAL and b"NULL together" in err()
    assert train(X=None) == EINVAL and b"null pointer" in err()
    assert train(ws=None) == EINVAL and b"null pointer" in err()
    for M, K, C in CITATION_SHAPES + ((3000, 602, 41),):
        need = lib.sgc_train_adam_workspace(M, K, C)
        assert train(M=M, K=K, C=C, ws_bytes=need - 1) == ENOMEM and b"workspace" in err()
    assert train(epochs=0) == 0  # valid arguments, nothing to enqueue
