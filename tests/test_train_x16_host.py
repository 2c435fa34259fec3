"""The 16-bit-feature training entries on a GPU-less host: the seven symbols
are declared, exported and bound; every argument error returns before any
device call; sgc_linear_xent_x16_kernel_name covers exactly what both existing
x16 name functions cover, and the workspace functions follow it; the drivers
parse the flag pairs that reach the fused 16-bit loops."""
import ctypes
import importlib.util
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sgc_linear_xent_x16_workspace", "sgc_linear_xent_x16", "sgc_linear_xent_x16_kernel_name",
         "sgc_train_adam_x16_workspace", "sgc_train_adam_x16", "sgc_train_lbfgs_x16_workspace",
         "sgc_train_lbfgs_x16")
BF16, F16 = 1, 2
EINVAL = 1
FAKE = 256 * 4096  # never dereferenced: the checks come first


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
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    from sgc_amd import build
    assert "xent16.hip" in build.SOURCES


def xent(lib, M=300, K=602, C=41, ldx=None, dt=BF16, X=FAKE):
    p = ctypes.c_void_p(FAKE)
    return lib.sgc_linear_xent_x16(ctypes.c_void_p(X), dt, K if ldx is None else ldx, p, p, p, M,
                                   K, C, p, p, p, p, 1 << 40, None)


def adam(lib, M=300, K=602, C=41, ldx=None, dt=BF16, X=FAKE, epochs=3):
    p = ctypes.c_void_p(FAKE)
    return lib.sgc_train_adam_x16(ctypes.c_void_p(X), dt, K if ldx is None else ldx, p, p, p, M, K,
                                  C, p, p, p, p, 0, epochs, 0.2, 0.9, 0.999, 1e-8, 5e-4, None, p,
                                  1 << 40, None)


def lbfgs(lib, M=300, K=602, C=41, ldx=None, dt=BF16, X=FAKE, steps=2):
    p = ctypes.c_void_p(FAKE)
    return lib.sgc_train_lbfgs_x16(ctypes.c_void_p(X), dt, K if ldx is None else ldx, p, p, p, M,
                                   K, C, p, steps, 1.0, 4, 5, 1e-7, 1e-9, None, None, p, 1 << 40,
                                   None)


BAD = {
    "unknown dtype": dict(dt=3),
    "fp32 dtype": dict(dt=0),
    "odd ldx": dict(ldx=603),
    "ldx < K": dict(ldx=600),
    "C = 49": dict(C=49),
    "2-B aligned base": dict(X=FAKE + 2),
    "M ldx 2 >= 2^31": dict(M=(2 ** 31) // (602 * 2) + 1),
}


@pytest.mark.parametrize("call", [xent, adam, lbfgs], ids=["xent", "adam", "lbfgs"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_return_before_any_device_call(lib, call, case):
    assert call(lib, **BAD[case]) == EINVAL, case
    text = lib.sgc_last_error()
    assert text and b"x16" in text, (case, text)


def test_nothing_to_enqueue_is_ok(lib):
    assert adam(lib, epochs=0) == 0
    assert lbfgs(lib, steps=0) == 0
    assert adam(lib, epochs=-1) == EINVAL and b"epochs=-1" in lib.sgc_last_error()
    assert lbfgs(lib, steps=-1) == EINVAL and b"steps=-1" in lib.sgc_last_error()


MS = (1, 16, 3000, (2 ** 31) // (602 * 2) + 1, 2 ** 29)
KS = (1, 2, 33, 64, 602, 1433, 1434, 3703, 70000)
CS = (1, 16, 17, 41, 48, 49, 64)


def test_name_function_is_the_intersection_and_workspaces_follow(lib):
    """No margin of its own: launch A needs the W image sgc_linear_x16 needs."""
    seen = {True: 0, False: 0}
    for M, K, C, dt, mis in itertools.product(MS, KS, CS, (BF16, F16, 0, 3), (0, 2)):
        for ldx in (K, K + 1, K + 6):
            X = ctypes.c_void_p(FAKE + mis)
            args = (M, K, ldx, C, X, dt)
            both = (lib.sgc_linear_x16_kernel_name(*args) != b"none" and
                    lib.sgc_linear_backward_x16_kernel_name(*args) != b"none")
            name = lib.sgc_linear_xent_x16_kernel_name(*args)
            assert (name != b"none") == both, (args, name)
            seen[both] += 1
            if both:
                assert lib.sgc_linear_xent_x16_workspace(M, K, C) > 0
                assert lib.sgc_train_adam_x16_workspace(M, K, C) > 0
                # (the L-BFGS state's own limit: C K + C <= 65,536 parameters)
                assert (lib.sgc_train_lbfgs_x16_workspace(M, K, C) > 0) == (C * K + C <= 65536)
    assert seen[True] > 100 and seen[False] > 100
    # 0 where no layout of (M, K, C) is covered: the tightest one is even ldx >= K, aligned
    for M, K, C in itertools.product(MS + (0,), KS + (0,), CS + (0,)):
        ldx = K + (K & 1)
        any_layout = M > 0 and K > 0 and C > 0 and lib.sgc_linear_xent_x16_kernel_name(
            M, K, ldx, C, ctypes.c_void_p(FAKE), BF16) != b"none"
        for f in (lib.sgc_linear_xent_x16_workspace, lib.sgc_train_adam_x16_workspace):
            assert (f(M, K, C) > 0) == any_layout, (M, K, C)
        assert (lib.sgc_train_lbfgs_x16_workspace(M, K, C) > 0) == \
            (any_layout and C * K + C <= 65536)


@pytest.mark.parametrize("M,K,ldx,C", [(3000, 602, 602, 41), (140, 1433, 1434, 7),
                                       (120, 3703, 3704, 6), (60, 500, 500, 3), (1, 2, 2, 1)])
def test_shapes_that_must_be_covered(lib, M, K, ldx, C):
    for dt in (BF16, F16):
        assert lib.sgc_linear_xent_x16_kernel_name(M, K, ldx, C, ctypes.c_void_p(FAKE),
                                                   dt) != b"none"


def load_driver(name):
    spec = importlib.util.spec_from_file_location("driver_" + name,
                                                  os.path.join(ROOT, "drivers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flags_parse():
    reddit = load_driver("reddit")
    a = reddit.parse(["--feature-dtype", "bfloat16", "--fused-lbfgs"])
    assert a.feature_dtype == "bfloat16" and a.fused_lbfgs
    citation = load_driver("citation")
    argv = ["--dataset", "cora", "--feature-dtype", "bfloat16", "--device-adam"]
    assert citation.get_citation_args(argv).dataset == "cora"
    a = citation.parse_own(argv)
    assert a.feature_dtype == "bfloat16" and a.device_adam
