"""Ragged feature widths through the SpMM's light, pairs and hub paths with
caller buffers in their worst layouts: idle lanes gather a line their
instruction's active lanes read (lane_lines.h) and are never stored, and rows
that are only 4-byte aligned are written and re-read with one vector access per
lane, never at or beyond column F.  All of it is a schedule, so every result
equals the CPU twin (sgc_propagate_f32_cpu) bit for bit."""
import functools
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 4096
K = 2
HEAVY, HUB = 64, 256  # forced thresholds: light <= 64 < pairs <= 256 < hub
WIDTHS = [602, 516, 132, 130, 90]
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgc_amd import _lib
    _lib.load()  # fails loudly if libsgc_amd.so is missing


@pytest.fixture()
def prop_mod():
    """sgc_amd.propagate with its schedule knobs restored afterwards."""
    mod = importlib.import_module("sgc_amd.propagate")
    saved = mod.COLUMN_GROUPS, mod.PAD_X0
    yield mod
    mod.COLUMN_GROUPS, mod.PAD_X0 = saved


@functools.lru_cache(maxsize=None)
def _graph():
    """4,096 rows, ~60 k nonzeros, ascending columns: mostly short rows, rows of
    33..64 nonzeros (cut by two column groups, still light), six rows of
    70..250 (pairs), one of 1,500 (hub), forty empty rows."""
    rng = np.random.default_rng(2024)
    deg = rng.integers(1, 24, size=N)
    deg[rng.choice(N, size=120, replace=False)] = rng.integers(33, 65, size=120)
    special = rng.choice(N, size=47, replace=False)
    deg[special[:6]] = [70, 97, 128, 129, 200, 250]
    deg[special[6]] = 1500
    deg[special[7:]] = 0
    deg[0], deg[N - 1] = 40, 0  # a cut light row first, an empty row last
    rp = np.zeros(N + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(N, size=d, replace=False)) for d in deg])
    va = rng.standard_normal(int(rp[-1])).astype(np.float32)
    return rp.astype(np.int32), ci.astype(np.int32), va


@pytest.fixture(scope="module")
def csr():
    from sgc_amd.propagate import DeviceCSR
    rp, ci, va = _graph()
    c = DeviceCSR.from_host_arrays(rp, ci, va, device=DEV)
    assert c.cols_ascending
    return c


@functools.lru_cache(maxsize=None)
def _case(F):
    """(X, S^K X by the CPU twin) at width F; computed once, never modified."""
    from sgc_amd.propagate import DeviceCSR, propagate
    rp, ci, va = _graph()
    X = np.random.default_rng(F).standard_normal((N, F)).astype(np.float32)
    want = propagate(DeviceCSR.from_host_arrays(rp, ci, va, device="cpu"),
                     torch.from_numpy(X), K).numpy()
    X.setflags(write=False)
    want.setflags(write=False)
    return X, want


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(csr, X, out):
    from sgc_amd.propagate import propagate
    propagate(csr, X, K, out=out, threshold=HEAVY, hub_threshold=HUB)
    torch.cuda.synchronize()


@pytest.mark.parametrize("G", [1, 2])
def test_plan_has_every_path(csr, G):
    """The forced thresholds give heavy (pairs) rows and a hub row in every
    column group, so the tests below run the light, pairs and hub paths."""
    for part in csr.groups_or_self(G):  # the groups propagate() launches
        pl = part.plan(0, N, HEAVY, HUB, 602)
        assert pl.n_hub >= 1 and pl.n_heavy > pl.n_hub, G


@pytest.mark.parametrize("pad", [True, None])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("F", WIDTHS)
def test_worst_alignment_flat_buffers(csr, prop_mod, F, G, pad):
    """`X` and `out` are [N, F] views one float into a flat buffer (4-byte
    aligned bases, rows F floats apart); X goes through the re-layout (pad =
    True) or straight into hop 1 (None: the rule, which says no here).  The
    floats before row 0 and after row N - 1 of `out` keep their sentinel."""
    prop_mod.COLUMN_GROUPS, prop_mod.PAD_X0 = G, pad
    X, want = _case(F)
    xflat = torch.full((N * F + 9,), float("nan"), dtype=torch.float32, device=DEV)
    Xd = xflat[1:1 + N * F].view(N, F)
    Xd.copy_(torch.tensor(X))
    oflat = torch.full((N * F + 9,), SENTINEL, dtype=torch.float32, device=DEV)
    out = oflat[1:1 + N * F].view(N, F)
    assert Xd.data_ptr() % 8 == 4 and out.data_ptr() % 8 == 4
    _run(csr, Xd, out)
    got = oflat.cpu().numpy()
    assert np.array_equal(_bits(got[1:1 + N * F]).reshape(N, F), _bits(want)), (F, G, pad)
    guard = np.concatenate([got[:1], got[1 + N * F:]])
    assert np.array_equal(_bits(guard), _bits(np.full(9, SENTINEL, np.float32))), (F, G, pad)
    assert np.array_equal(_bits(Xd.cpu().numpy()), _bits(X)), "X was written"


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("F", WIDTHS)
def test_gap_columns_keep_their_sentinel(csr, prop_mod, F, G):
    """`out` is the [:, :F] view of an [N, F + 3] buffer: no store (and, with
    two groups, no partial-sum reload that matters) reaches column F or beyond."""
    prop_mod.COLUMN_GROUPS = G
    X, want = _case(F)
    buf = torch.full((N, F + 3), SENTINEL, dtype=torch.float32, device=DEV)
    _run(csr, torch.tensor(X).to(DEV), buf[:, :F])
    got = buf.cpu().numpy()
    assert np.array_equal(_bits(got[:, :F]), _bits(want)), (F, G)
    assert np.array_equal(_bits(got[:, F:]), _bits(np.full((N, 3), SENTINEL, np.float32))), (F, G)


@pytest.mark.parametrize("pad", [True, None])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("F", WIDTHS)
def test_poisoned_gap_columns_of_x(csr, prop_mod, F, G, pad):
    """`X` is the [:, :F] view of an [N, F + 3] buffer whose gap columns hold
    NaN: no idle lane's load enters a chain."""
    prop_mod.COLUMN_GROUPS, prop_mod.PAD_X0 = G, pad
    X, want = _case(F)
    buf = torch.full((N, F + 3), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :F] = torch.tensor(X).to(DEV)
    out = torch.full((N, F), SENTINEL, dtype=torch.float32, device=DEV)
    _run(csr, buf[:, :F], out)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (F, G, pad)
