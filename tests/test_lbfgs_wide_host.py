"""Wide L-BFGS checks that need no GPU: the new exports and their argument
rejections, the documented state size, and the numpy fp64 model of the
Gram-form iteration (tests/lbfgs_wide_model.py) held to `ref_step` of
tests/test_lbfgs_host.py, with mutants of the model shown to be caught.

(The rejection of numels that do not sum to the state's n needs a state that
sgc_lbfgs_wide_init accepted, so a device: tests/test_gpu_lbfgs_wide.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lbfgs_wide_model import MUTANTS, _bumpy, run_model
from test_lbfgs_host import (CASES, STOP_MAX_ITER, _grid, assert_not_borderline, case_x0,
                             quadratic, ref_step)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE_CASES = dict(CASES)
# the ring (3 slots) is full from the fifth iteration on and wraps twice
WIDE_CASES["full_ring"] = dict(shapes=[(40,)], f=quadratic(40),
                               opts=dict(max_iter=8, max_eval=20, history_size=3), steps=1,
                               reasons=[STOP_MAX_ITER])
# non-convex: the pair of the fifth iteration has ys < 0 and is rejected while
# the ring is full; five more iterations follow on the kept history
WIDE_CASES["reject_full_ring"] = dict(shapes=[(16,)], f=_bumpy,
                                      opts=dict(max_iter=10, max_eval=40, history_size=3), steps=1,
                                      reasons=[STOP_MAX_ITER])


def wide_x0(name):
    if name == "reject_full_ring":
        return _grid(16, -2.0, 2.0)
    if name == "full_ring":
        return _grid(40, -0.5, 0.5)
    return case_x0(CASES[name])


def run_ref_wide(name, trace=None):
    case = WIDE_CASES[name]
    x, st, reasons = wide_x0(name).clone(), {}, []
    for _ in range(case["steps"]):
        reasons.append(ref_step(case["f"], x, st, trace=trace, **case["opts"]))
    return x, st, reasons


def rel_diff(a, b):
    a, b = np.nan_to_num(a, nan=1234.5), np.nan_to_num(b, nan=1234.5)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            trace = []
            cache[name] = run_ref_wide(name, trace) + (trace,)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(WIDE_CASES))
def test_gram_model_is_ref_step(refs, name):
    """Parameters to 1e-12 (relative to the largest), equal statuses."""
    x64, st, reasons, trace = refs(name)
    assert reasons == WIDE_CASES[name]["reasons"]
    assert_not_borderline(trace)
    x, model, statuses = run_model(WIDE_CASES[name], wide_x0(name))
    assert [s[4] for s in statuses] == reasons
    assert statuses[-1][:2] == (st["n_iter"], st["func_evals"])
    assert statuses[-1][5] == len(st.get("old_dirs") or [])
    err = rel_diff(x, x64.numpy())
    print(f"gram model vs ref_step {name}: {err:.3e}")
    assert err <= 1e-12
    # the incrementally kept Gram block is the block of the rows as they lie
    G, full = model.G, model.sync_gram()
    scale = max(np.abs(np.nan_to_num(full)).max(), 1e-300)
    assert np.abs(np.nan_to_num(G) - np.nan_to_num(full)).max() <= 1e-12 * scale


def test_new_cases_do_what_they_are_named_for():
    _, model, _ = run_model(WIDE_CASES["full_ring"], wide_x0("full_ring"))
    assert model.pushes == 7 and model.h == 3 and model.rejects_full == 0
    _, model, _ = run_model(WIDE_CASES["reject_full_ring"], wide_x0("reject_full_ring"))
    assert model.rejects_full >= 1 and model.h == 3 and model.pushes >= 4


@pytest.mark.parametrize("mutant,name", [("evicted_gram_kept", "full_ring"),
                                         ("stale_g_row", "reject_full_ring"),
                                         ("stage_into_ring", "reject_full_ring"),
                                         ("hdiag_on_reject", "reject_full_ring")])
def test_mutants_are_caught(refs, mutant, name):
    assert mutant in MUTANTS
    x64, st, reasons, _ = refs(name)
    x, model, statuses = run_model(WIDE_CASES[name], wide_x0(name), mutant=mutant)
    err = rel_diff(x, x64.numpy())
    print(f"mutant {mutant} on {name}: {err:.3e}")
    assert err > 1e-9 or [s[4] for s in statuses] != reasons


# --- C ABI ------------------------------------------------------------------------

NEW = ("sgc_lbfgs_wide_workspace", "sgc_lbfgs_wide_init", "sgc_lbfgs_wide_begin_step",
       "sgc_lbfgs_wide_iterate_f32", "sgc_lbfgs_wide_read_status", "sgc_lbfgs_wide_sync_gram",
       "sgc_lbfgs_wide_l2_f32", "sgc_train_lbfgs_wide_workspace", "sgc_train_lbfgs_wide_f32")


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import build
    build.build(verbose=False)
    from sgc_amd import _lib
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    from sgc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    narrow, wide = _lib.SIGNATURES["sgc_lbfgs_iterate_f32"], \
        _lib.SIGNATURES["sgc_lbfgs_wide_iterate_f32"]
    assert narrow == wide
    for a, b in (("sgc_lbfgs_workspace", "sgc_lbfgs_wide_workspace"),
                 ("sgc_lbfgs_init", "sgc_lbfgs_wide_init"),
                 ("sgc_lbfgs_begin_step", "sgc_lbfgs_wide_begin_step"),
                 ("sgc_lbfgs_read_status", "sgc_lbfgs_wide_read_status")):
        assert _lib.SIGNATURES[a] == _lib.SIGNATURES[b]
    t_narrow, t_wide = _lib.SIGNATURES["sgc_train_lbfgs_f32"], \
        _lib.SIGNATURES["sgc_train_lbfgs_wide_f32"]
    assert t_wide[1] == t_narrow[1][:15] + [ctypes.c_double] + t_narrow[1][15:]  # l2
    assert "lbfgs_wide.hip" in __import__("sgc_amd.build", fromlist=["SOURCES"]).SOURCES


def documented_bytes(n, m):
    """include/sgc_amd.h's layout of the state."""
    up = lambda v, a: (v + a - 1) // a * a  # noqa: E731
    ld = up(n, 32)
    tile = 1024 if ld <= 262144 else (2048 if ld <= 1048576 else 4096)
    B, P = 2 * m + 1, 16 + 6 * m
    return (256 + up(4 * m, 256) + (4 + 2 * m) * ld * 4 + up(B * 8, 256) + up(P * 8, 256) +
            up(B * B * 8, 256) + up(-(-ld // tile) * P * 8, 256))


def test_workspace_size_and_range(lib):
    for n, m in ((1, 1), (65536, 100), (65537, 100), (2 ** 21, 4), (1232060, 100), (69333, 1024),
                 (262144, 3), (262145, 3), (1048577, 2)):
        assert lib.sgc_lbfgs_wide_workspace(n, m) == documented_bytes(n, m) > 0, (n, m)
    # the narrow prefix: header | ro | d | prev_g | S | Y
    assert lib.sgc_lbfgs_wide_workspace(24723, 100) > lib.sgc_lbfgs_workspace(24723, 100)
    for n, m, text in ((0, 10, b"n=0 < 1"), (2 ** 31 - 1, 10, b">= 2^31 - 1"),
                       (10, 0, b"history_size=0 < 1"), (10, 1025, b"history_size=1025 > 1024")):
        assert lib.sgc_lbfgs_wide_workspace(n, m) == 0
        assert text in lib.sgc_last_error(), (n, m, lib.sgc_last_error())


def test_argument_rejections_before_any_device_call(lib):
    EINVAL, ERANGE, ENOMEM = 1, 2, 4
    fake = ctypes.c_void_p(256 * 4096)  # never dereferenced: the checks come first

    def err():
        return lib.sgc_last_error()
    init = lib.sgc_lbfgs_wide_init
    assert init(None, 1 << 20, 10, 5, None) == EINVAL and b"null state" in err()
    assert init(fake, 1 << 20, 0, 5, None) == EINVAL and b"n=0 < 1" in err()
    assert init(fake, 1 << 20, 10, 0, None) == EINVAL and b"history_size=0 < 1" in err()
    assert init(fake, 1 << 20, 10, 1025, None) == ERANGE and b"1025" in err()
    assert init(fake, 16, 10, 5, None) == ENOMEM and b"bytes" in err()  # a short state
    assert init(fake, documented_bytes(65537, 5) - 1, 65537, 5, None) == ENOMEM
    assert init(ctypes.c_void_p(256 * 4096 + 4), 1 << 20, 10, 5, None) == EINVAL and \
        b"aligned" in err()
    assert lib.sgc_lbfgs_wide_begin_step(None, None) == EINVAL and b"null state" in err()
    assert lib.sgc_lbfgs_wide_sync_gram(None, None) == EINVAL and b"null state" in err()
    assert lib.sgc_lbfgs_wide_sync_gram(fake, None) == EINVAL and b"not initialised" in err()
    out = (ctypes.c_int64 * 6)()
    assert lib.sgc_lbfgs_wide_read_status(None, out, None) == EINVAL and b"null state" in err()
    assert lib.sgc_lbfgs_wide_read_status(fake, None, None) == EINVAL and b"null out_host" in err()

    ptrs = (ctypes.c_void_p * 17)()
    numels = (ctypes.c_int64 * 17)(*([40000] * 17))

    def iterate(state, nt, p=ptrs, g=ptrs, k=numels, max_iter=20):
        return lib.sgc_lbfgs_wide_iterate_f32(state, nt, p, g, k, None, 1.0, max_iter, 25, 1e-7,
                                              1e-9, None)
    assert iterate(None, 2) == EINVAL and b"null state" in err()
    for nt in (0, 17, -1):  # more than 16 tensors
        assert iterate(fake, nt) == EINVAL and b"outside 1..16" in err()
    assert iterate(fake, 2, p=None) == EINVAL and b"null pointer table" in err()
    assert iterate(fake, 2, max_iter=0) == EINVAL and b"max_iter" in err()
    neg = (ctypes.c_int64 * 2)(4, -1)
    assert iterate(fake, 2, k=neg) == EINVAL and b"numels[1]=-1" in err()
    zero = (ctypes.c_int64 * 2)(0, 0)
    assert iterate(fake, 2, k=zero) == EINVAL and b"n=0 < 1" in err()
    huge = (ctypes.c_int64 * 2)(2 ** 31 - 2, 1)
    assert iterate(fake, 2, k=huge) == ERANGE and b"2^31" in err()
    # 80,000 parameters pass the size checks; the state was never initialised
    assert iterate(fake, 2) == EINVAL and b"not initialised" in err()
    assert lib.sgc_lbfgs_wide_l2_f32(fake, fake, fake, 10, 1e-3, fake, None) == EINVAL and \
        b"not initialised" in err()
    assert lib.sgc_lbfgs_wide_l2_f32(fake, None, fake, 10, 1e-3, fake, None) == EINVAL


def test_train_rejections_before_any_device_call(lib):
    EINVAL, ENOMEM = 1, 4
    fake = ctypes.c_void_p(256 * 4096)

    def err():
        return lib.sgc_last_error()

    def train(M=37, K=2100, C=33, ldx=None, steps=3, ws_bytes=None, state=fake, max_iter=20):
        need = lib.sgc_train_lbfgs_wide_workspace(M, K, min(C, 64))
        return lib.sgc_train_lbfgs_wide_f32(
            fake, K if ldx is None else ldx, fake, fake, fake, M, K, C, state, steps, 1.0,
            max_iter, 25, 1e-7, 1e-9, 5e-4, None, None, fake, need if ws_bytes is None else
            ws_bytes, None)
    assert lib.sgc_train_lbfgs_wide_workspace(37, 2100, 33) > (33 * 2100 + 33) * 4
    assert lib.sgc_train_lbfgs_wide_workspace(37, 2100, 65) == 0
    assert train(C=65) == EINVAL and b"C <= 64" in err()
    assert train(ldx=2099) == EINVAL and b"ldx >= K" in err()
    assert train(steps=-1) == EINVAL and b"steps=-1" in err()
    assert train(max_iter=0) == EINVAL and b"max_iter" in err()
    assert train(ws_bytes=16) == ENOMEM and b"workspace 16 <" in err()
    assert train(state=None) == EINVAL and b"null pointer" in err()
    assert train(steps=0) == 0  # SGC_OK: nothing to do, nothing touched
    assert train() == EINVAL and b"not initialised" in err()


def test_wide_keyword_keeps_the_constructor():
    """LBFGS(..., wide=True) without a new __init__ parameter; CPU parameters
    take torch's step either way."""
    from sgc_amd.optim import LBFGS
    p = torch.zeros(70000, requires_grad=True)
    opt = LBFGS([p], max_iter=3, wide=True)
    assert opt.wide and not opt.device_path()
    assert not LBFGS([p]).wide

    def closure():
        opt.zero_grad()
        loss = ((p - 1.0) ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)
    assert opt._dev_state is None and opt.last_status is None  # torch's own step ran
    assert opt.state[p]["n_iter"] >= 1 and float(p.detach().abs().max()) > 0


def test_textsgc_model_and_cpu_training_are_the_reference_loop():
    """CPU tensors run torch throughout: train_linear equals the literal loop
    of torch.optim.LBFGS on the reference closure bit for bit."""
    from sgc_amd import textsgc
    torch.manual_seed(3)
    model = textsgc.SGC(50, 4)
    assert model.W.bias is None and textsgc.SGC(5, 2, bias=True).W.bias is not None
    g = torch.Generator().manual_seed(1)
    feats = {k: torch.rand(m, 50, generator=g) for k, m in (("train", 60), ("val", 20))}
    labels = {k: torch.randint(0, 4, (v.shape[0],), generator=g) for k, v in feats.items()}
    twin = textsgc.SGC(50, 4)
    twin.load_state_dict(model.state_dict())
    acc, out, seconds = textsgc.train_linear(model, feats, labels, 5e-4, epochs=2)
    opt = torch.optim.LBFGS(twin.parameters())

    def closure():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(twin(feats["train"]), labels["train"]) + \
            0.5 * 5e-4 * (twin.W.weight ** 2).sum()
        loss.backward()
        return loss
    for _ in range(2):
        opt.step(closure)
    assert out is model and seconds > 0
    assert torch.equal(model.W.weight, twin.W.weight)
    res = textsgc.eval_linear(model, feats["val"], labels["val"])
    assert res["accuracy"] == acc and 0.0 <= acc <= 1.0 and res["loss"] > 0
    # binary: one output, float labels
    bm = textsgc.SGC(50, 1)
    bl = {k: v.gt(1).float() for k, v in labels.items()}
    acc, _, _ = textsgc.train_linear(bm, feats, bl, 0.0, epochs=1, binary=True)
    assert acc == textsgc.eval_linear(bm, feats["val"], bl["val"], binary=True)["accuracy"]
