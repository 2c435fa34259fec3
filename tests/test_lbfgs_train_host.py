"""Fused L-BFGS training (sgc_train_lbfgs_f32, LBFGS.run_steps) checks that
need no GPU: the new symbols, the workspace sizes, the argument rejections of
the C entry point, the CPU fallback of run_steps against torch.optim.LBFGS and
the driver's flag."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import build
    build.build(verbose=False)
    from sgc_amd import _lib
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from sgc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sgc_train_lbfgs_workspace", "sgc_train_lbfgs_f32"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["sgc_train_lbfgs_f32"][1]) == 20
    assert "#define SGC_ABI_VERSION 1" in hdr


def test_workspace_sizes(lib):
    for M, K, C in ((1, 1, 1), (70, 33, 3), (300, 602, 41), (40, 1023, 64), (152410, 602, 41)):
        n = C * K + C
        assert lib.sgc_train_lbfgs_workspace(M, K, C) >= \
            lib.sgc_linear_xent_workspace(M, K, C) + n * 4
    for M, K, C in ((0, 10, 3), (10, 0, 3), (10, 10, 0), (10, 10, 65), (10, 1025, 64)):
        assert lib.sgc_train_lbfgs_workspace(M, K, C) == 0


def test_argument_rejections_before_any_device_call(lib):
    """Fake device pointers throughout: every call stops at its argument
    checks with its code and text."""
    EINVAL, ERANGE, ENOMEM = 1, 2, 4
    fake = ctypes.c_void_p(256 * 4096)  # never dereferenced: the checks come first

    def err():
        return lib.sgc_last_error()

    def train(M=300, K=602, C=41, ldx=None, X=fake, W=fake, b=fake, y=fake, state=fake, steps=2,
              max_iter=20, ws=fake, ws_bytes=1 << 30):
        return lib.sgc_train_lbfgs_f32(X, K if ldx is None else ldx, W, b, y, M, K, C, state, steps,
                                       1.0, max_iter, 25, 1e-7, 1e-9, None, None, ws, ws_bytes,
                                       None)
    assert train(steps=-1) == EINVAL and b"steps=-1 < 0" in err()
    assert train(C=0) == EINVAL and b"C=0" in err()
    assert train(C=65) == EINVAL and b"C=65" in err()
    assert train(M=0) == EINVAL and b"M=0" in err()
    assert train(K=0) == EINVAL and b"K=0" in err()
    assert train(ldx=601) == EINVAL and b"ldx=601" in err()
    assert train(max_iter=0) == EINVAL and b"max_iter=0 < 1" in err()
    for k in ("X", "W", "y", "state", "ws"):
        assert train(**{k: None}) == EINVAL and b"null pointer" in err(), k
    assert train(X=ctypes.c_void_p(256 * 4096 + 2)) == EINVAL and b"4-B aligned" in err()
    assert train(K=1024, C=64) == ERANGE and b"n=65600 > 65536" in err()
    assert train(K=1024, C=64, b=None) == EINVAL and b"not initialised" in err()  # n = 65536 fits
    assert train(M=4, K=8, C=2, ldx=1 << 29) == ERANGE and b"31-bit" in err()
    for M, K, C in ((1, 1, 1), (300, 602, 41), (3000, 602, 41)):
        need = lib.sgc_train_lbfgs_workspace(M, K, C)
        assert train(M=M, K=K, C=C, ws_bytes=need - 1) == ENOMEM and b"workspace" in err()
    # a state sgc_lbfgs_init never saw
    assert train() == EINVAL and b"not initialised" in err()
    assert train(steps=0) == 0  # valid arguments, nothing to enqueue


def small_problem(M=37, K=65, C=5, seed=0):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=gen)
    y = torch.randint(0, C, (M,), generator=gen)
    return X, y


@pytest.mark.parametrize("ignored", [False, True])
def test_cpu_run_steps_is_torch_lbfgs_bit_for_bit(ignored):
    from sgc_amd.models import SGC
    from sgc_amd.optim import LBFGS
    X, y = small_problem()
    if ignored:
        y[::5] = -100
    models = [SGC(X.shape[1], 5), SGC(X.shape[1], 5)]
    models[1].load_state_dict(models[0].state_dict())
    ours = LBFGS(models[0].parameters(), lr=1, max_iter=6)
    got = ours.run_steps(models[0], X, y, 3)
    theirs = torch.optim.LBFGS(models[1].parameters(), lr=1, max_iter=6)

    def closure():
        theirs.zero_grad()
        loss = F.cross_entropy(models[1](X), y)
        loss.backward()
        return loss
    want = torch.stack([theirs.step(closure).detach() for _ in range(3)])
    assert got.shape == (3,) and torch.equal(got, want)
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p.detach(), q.detach())
    a, b = ours.state[ours._params[0]], theirs.state[theirs._params[0]]
    assert (a["n_iter"], a["func_evals"]) == (b["n_iter"], b["func_evals"])
    assert ours.step_statuses == [None] * 3 and ours.last_status is None
    assert not ours.device_path()


def test_cpu_run_steps_zero_steps_and_bad_arguments():
    from sgc_amd.models import SGC
    from sgc_amd.optim import LBFGS
    X, y = small_problem()
    model = SGC(X.shape[1], 5)
    opt = LBFGS(model.parameters(), lr=1, max_iter=4)
    before = [p.detach().clone() for p in model.parameters()]
    assert opt.run_steps(model, X, y, 0) is None
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert len(opt.state) == 0
    with pytest.raises(ValueError):
        opt.run_steps(model, X, y, -1)
    bad = y.clone()
    bad[3] = 5
    with pytest.raises(IndexError):
        opt.run_steps(model, X, bad, 1)


def test_fused_lbfgs_flag_parses():
    spec = importlib.util.spec_from_file_location("reddit_driver",
                                                  os.path.join(ROOT, "drivers", "reddit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse(["--fused-lbfgs"]).fused_lbfgs is True
    args = mod.parse([])
    assert args.fused_lbfgs is False and args.device_lbfgs is False
    assert mod.parse(["--device-lbfgs"]).fused_lbfgs is False
