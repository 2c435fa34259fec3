"""bfloat16 / float16 feature storage on the GPU (sgc_spmm_csr_x16).

Contract: 16 bits in memory, fp32 everywhere else -- each hop is the fp32
kernels' single sequential FMA chain on the exactly widened features, rounded
to nearest even once per stored element.  So every result here is compared
bit for bit (raw 16-bit patterns) with the emulation

    X_{k+1} = fp32_spmm(S, X_k.float()).to(T)

where fp32_spmm is the oracle (the CPU restatement of torch.spmm's arithmetic)
and .to(T) is torch's CPU conversion; the plan is a schedule only.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 0x7B7B  # a 16-bit pattern no result below equals by construction of the checks


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgc_amd import _lib
    _lib.load()


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    if got.dtype == torch.float32:
        return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32),
                                                       want.contiguous().view(torch.int32))
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits16(got),
                                                                               bits16(want))


@functools.lru_cache(maxsize=None)
def graph_a():
    """n = 3000: row 0 with 900 nonzeros, row 7 with 300, 15,000 random pairs
    (the fp32 suite's _narrow_case graph)."""
    from sgc_amd import graphs
    rng = np.random.default_rng(11)
    n = 3000
    lo = np.concatenate([np.zeros(900, np.int64), np.full(300, 7, np.int64),
                         rng.integers(0, n, 15000)])
    hi = np.concatenate([np.arange(100, 1000), np.arange(1000, 1300), rng.integers(0, n, 15000)])
    keep = lo != hi
    a, b = np.minimum(lo, hi)[keep], np.maximum(lo, hi)[keep]
    key = np.unique(a * n + b)
    return graphs.aug_norm_csr_from_pairs(n, key // n, key % n)


@functools.lru_cache(maxsize=None)
def graph_b():
    """n = 9000: hub rows of 7,000 / 3,001 / 2,881 nonzeros, 20,000 random pairs
    (test_long_hub_rows_bit_exact's graph)."""
    from sgc_amd import graphs
    rng = np.random.default_rng(12)
    n = 9000
    u = [np.zeros(7000, np.int64), np.full(3001, 1, np.int64), np.full(2881, 2, np.int64)]
    v = [np.arange(1000, 8000), np.arange(3000, 6001), np.arange(5000, 7881)]
    ru, rv = rng.integers(3, n, 20000), rng.integers(3, n, 20000)
    keep = ru != rv
    lo = np.concatenate(u + [np.minimum(ru, rv)[keep]])
    hi = np.concatenate(v + [np.maximum(ru, rv)[keep]])
    key = np.unique(lo * n + hi)
    return graphs.aug_norm_csr_from_pairs(n, key // n, key % n)


def host_csr(S):
    return (np.ascontiguousarray(S.row_ptr, np.int32), np.ascontiguousarray(S.col_idx, np.int32),
            np.ascontiguousarray(S.val, np.float32))


def emulate(oracle, csr, X16, K, last_fp32=False):
    rp, ci, va = csr
    X = X16
    for h in range(K):
        Y = torch.from_numpy(oracle.spmm_csr(rp, ci, va, X.float().numpy(), 0, rp.size - 1))
        X = Y if (last_fp32 and h == K - 1) else Y.to(X16.dtype)
    return X


def features(n, F, dtype, seed):
    return torch.from_numpy(
        np.random.default_rng(seed).standard_normal((n, F)).astype(np.float32)).to(dtype)


def in_line_rows(X16):
    """X on the device in 128-B rows (64 elements), as a [:, :F] view."""
    n, F = X16.shape
    Xd = torch.zeros((n, (F + 63) // 64 * 64), dtype=X16.dtype, device=DEV)[:, :F]
    Xd.copy_(X16)
    return Xd


def device_csr(S):
    from sgc_amd.propagate import DeviceCSR
    return DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [1, 7, 8, 9, 63, 64, 65, 130, 256, 511, 512, 513, 602])
def test_widths_bit_exact(oracle, F, dtype):
    """The edges of a lane's 8 elements, of a 128-B line and of a wave's
    512-element span; light + heavy + hub rows (40, 500) and light rows only."""
    from sgc_amd.propagate import propagate
    S = graph_a()
    n = S.row_ptr.size - 1
    X = features(n, F, dtype, F)
    want = emulate(oracle, host_csr(S), X, 2)
    csr, Xd = device_csr(S), in_line_rows(X)
    for th, hub in ((40, 500), (10**9, 10**9)):
        out = propagate(csr, Xd, 2, threshold=th, hub_threshold=hub)
        torch.cuda.synchronize()
        assert out.dtype == dtype and same_bits(out, want), (F, th, hub)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [64, 130, 192])
@pytest.mark.parametrize("hub_chunk", [32, 64])
@pytest.mark.parametrize("hub_loaders", [15, 7])
def test_hub_kernel_bit_exact(oracle, F, hub_chunk, hub_loaders, dtype):
    """Hub rows of 7,000 / 3,001 / 2,881 nonzeros on the LDS-staged hub kernel
    with 16-bit gathers: several unrolled rounds, the register ring's wrap,
    ragged last rounds."""
    from sgc_amd import _lib
    from sgc_amd.propagate import propagate
    S = graph_b()
    n = S.row_ptr.size - 1
    X = features(n, F, dtype, F + hub_chunk)
    want = emulate(oracle, host_csr(S), X, 2)
    lib = _lib.load()
    _lib.check(lib.sgc_set_tuning(b"hub_chunk", hub_chunk), "set_tuning")
    _lib.check(lib.sgc_set_tuning(b"hub_loaders", hub_loaders), "set_tuning")
    try:
        csr = device_csr(S)
        assert csr.plan(0, n, 64, 1000, F).n_hub == 3
        out = propagate(csr, in_line_rows(X), 2, threshold=64, hub_threshold=1000)
        torch.cuda.synchronize()
        assert same_bits(out, want)
    finally:
        lib.sgc_set_tuning(b"hub_chunk", 0)
        lib.sgc_set_tuning(b"hub_loaders", 15)


@pytest.mark.parametrize("dtype", DTYPES)
def test_schedule_never_changes_bits(oracle, dtype):
    from sgc_amd import _lib
    from sgc_amd.propagate import propagate
    S = graph_a()
    n, F = S.row_ptr.size - 1, 130
    X = features(n, F, dtype, 5)
    want = emulate(oracle, host_csr(S), X, 2)
    csr, Xd = device_csr(S), in_line_rows(X)
    lib = _lib.load()
    try:
        for rpw in (0, 1, 2, 4):
            _lib.check(lib.sgc_set_tuning(b"rows_per_wave", rpw), "set_tuning")
            for th, hub in ((0, 0), (1, 7), (7, 7), (63, 500), (0, 10**9), (10**9, 10**9),
                            (2048, 4096)):
                out = propagate(csr, Xd, 2, threshold=th, hub_threshold=hub)
                torch.cuda.synchronize()
                assert same_bits(out, want), (rpw, th, hub)
    finally:
        lib.sgc_set_tuning(b"rows_per_wave", 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [130, 602])
def test_lane_width_knobs_never_change_bits(oracle, F, dtype):
    """x16_vec (16- / 8- / 4- / 2-byte lanes: one to ten feature slices at
    F = 602) and x16_step are schedules: the same bits, hub + heavy + light."""
    from sgc_amd import _lib
    from sgc_amd.propagate import propagate
    S = graph_a()
    n = S.row_ptr.size - 1
    X = features(n, F, dtype, F + 7)
    want = emulate(oracle, host_csr(S), X, 2)
    csr, Xd = device_csr(S), in_line_rows(X)
    lib = _lib.load()
    try:
        for vec in (0, 8, 4, 2, 1):
            for step in (0, 4, 8):
                _lib.check(lib.sgc_set_tuning(b"x16_vec", vec), "set_tuning")
                _lib.check(lib.sgc_set_tuning(b"x16_step", step), "set_tuning")
                out = propagate(csr, Xd, 2, threshold=40, hub_threshold=500)
                torch.cuda.synchronize()
                assert same_bits(out, want), (vec, step)
    finally:
        lib.sgc_set_tuning(b"x16_vec", 0)
        lib.sgc_set_tuning(b"x16_step", 0)


@functools.lru_cache(maxsize=None)
def graph_a_with_empty_rows():
    """Graph A with the nonzeros of rows 10, 11 and 2299 removed."""
    rp, ci, va = host_csr(graph_a())
    deg = np.diff(rp.astype(np.int64))
    keep = np.ones(ci.size, bool)
    for r in (10, 11, 2299):
        keep[rp[r]:rp[r + 1]] = False
        deg[r] = 0
    rp2 = np.zeros(rp.size, np.int64)
    np.cumsum(deg, out=rp2[1:])
    return rp2.astype(np.int32), ci[keep].copy(), va[keep].copy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [602, 65])
def test_layouts_and_row_ranges(oracle, F, dtype):
    """Caller layouts through spmm: ld = F, F + 3 (odd: 2-byte loads) and F
    rounded up to 64, and a column-slice view whose base is only 2-B aligned;
    whole and partial row ranges.  Nothing outside [r0, r1) x [0, F) of the
    output buffer changes, every element inside is written, rows without
    nonzeros get +0."""
    from sgc_amd.propagate import DeviceCSR, spmm
    rp, ci, va = graph_a_with_empty_rows()
    n = rp.size - 1
    X = features(n, F, dtype, F + 1)
    want = emulate(oracle, (rp, ci, va), X, 1)
    assert bits16(want[10]).eq(0).all() and bits16(want[2299]).eq(0).all()  # +0, not -0
    csr = DeviceCSR.from_host_arrays(rp, ci, va)
    r64 = (F + 63) // 64 * 64
    layouts = []
    for ld in (F, F + 3, r64):
        buf = torch.zeros((n, ld), dtype=dtype, device=DEV)
        layouts.append((f"ld={ld}", buf[:, :F], ld))
    big = torch.zeros((n, F + 8), dtype=dtype, device=DEV)
    layouts.append(("slice", big[:, 3:3 + F], F + 3))
    assert layouts[-1][1].data_ptr() % 4 == 2
    for name, Xd, ldo in layouts:
        Xd.copy_(X)
        for r0, r1 in ((0, n), (5, 2300)):
            obuf = torch.empty((n, ldo), dtype=dtype, device=DEV)
            obuf.view(torch.int16).fill_(SENTINEL)
            spmm(csr, Xd, r0, r1, out=obuf[r0:r1, :F], threshold=40, hub_threshold=500)
            torch.cuda.synchronize()
            got = obuf.cpu()
            assert same_bits(got[r0:r1, :F], want[r0:r1]), (name, r0, r1)
            raw = got.view(torch.int16)
            assert raw[:r0].eq(SENTINEL).all() and raw[r1:].eq(SENTINEL).all(), (name, r0, r1)
            assert raw[:, F:].eq(SENTINEL).all(), (name, r0, r1)
            y = spmm(csr, Xd, r0, r1, use_plan=False)
            torch.cuda.synchronize()
            assert same_bits(y, want[r0:r1]), (name, r0, r1, "no plan")


def _column_split(csr, bounds):
    """The nonzeros split by column range [bounds[g], bounds[g+1]): one CSR per
    range over the same rows (each row's runs stay in CSR order)."""
    rp, ci, va = (np.asarray(csr[0], np.int64), csr[1], csr[2])
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    grp = np.searchsorted(np.asarray(bounds), ci, side="right") - 1
    out = []
    for g in range(len(bounds) - 1):
        m = grp == g
        sub_rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(row[m], minlength=n), out=sub_rp[1:])
        out.append((sub_rp.astype(np.int32), ci[m], va[m]))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [130, 602])
def test_fp32_output_and_accumulate(oracle, F, dtype):
    from sgc_amd.propagate import SPMM_ACCUMULATE, DeviceCSR, propagate, spmm
    S = graph_a()
    csr_h = host_csr(S)
    n = csr_h[0].size - 1
    X = features(n, F, dtype, F + 2)
    want1 = emulate(oracle, csr_h, X, 1, last_fp32=True)
    csr, Xd = device_csr(S), in_line_rows(X)
    for th, hub in ((40, 500), (10**9, 10**9)):
        y = spmm(csr, Xd, threshold=th, hub_threshold=hub, out_dtype=torch.float32)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and same_bits(y, want1), (th, hub)
        # one plain pass over column block 0, accumulate passes over blocks 1..
        out = torch.full((n, F), float("nan"), device=DEV)
        for g, t in enumerate(_column_split(csr_h, [0, 700, 1100, 1600, n])):
            spmm(DeviceCSR.from_host_arrays(*t, n_cols=n), Xd, out=out, threshold=th,
                 hub_threshold=hub, flags=SPMM_ACCUMULATE if g else 0)
        torch.cuda.synchronize()
        assert same_bits(out, want1), (th, hub, "accumulate")
    out = propagate(csr, Xd, 2, out_dtype=torch.float32, threshold=40, hub_threshold=500)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32
    assert same_bits(out, emulate(oracle, csr_h, X, 2, last_fp32=True))
    with pytest.raises(TypeError):  # a chain is never continued from a rounded store
        spmm(csr, Xd, out=torch.zeros((n, F), dtype=dtype, device=DEV), flags=SPMM_ACCUMULATE)


@pytest.mark.parametrize("dtype,scale", [(torch.float16, 1e-6), (torch.bfloat16, 1e-38),
                                         (torch.float16, 3e4)])
def test_rounding_edges(oracle, dtype, scale):
    """Outputs straddling T's smallest normal (subnormal results), fp16 chains
    overflowing to inf, and one X row of +-inf and NaN: bit-equal where the
    emulation is finite or infinite, NaN where it is NaN."""
    from sgc_amd.propagate import propagate
    S = graph_a()
    n, F = S.row_ptr.size - 1, 64
    Xf = np.random.default_rng(3).standard_normal((n, F)).astype(np.float32) * np.float32(scale)
    X = torch.from_numpy(Xf).to(dtype)
    X[1500, 0::3] = float("inf")
    X[1500, 1::3] = float("-inf")
    X[1500, 2::3] = float("nan")
    want = emulate(oracle, host_csr(S), X, 2)
    tiny = torch.finfo(dtype).tiny
    mag = want.float().abs()
    if scale < 1:  # subnormal results of T are there to be compared
        assert ((mag > 0) & (mag < tiny)).any()
    else:
        assert torch.isinf(want).any() and torch.isfinite(want).any()
    csr = device_csr(S)
    for th, hub in ((40, 500), (10**9, 10**9)):
        out = propagate(csr, in_line_rows(X), 2, threshold=th, hub_threshold=hub).cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(out), nan), (th, hub)
        assert torch.equal(bits16(out)[~nan], bits16(want)[~nan]), (th, hub)


@pytest.mark.parametrize("dtype", DTYPES)
def test_public_call(tiny_cases, oracle, dtype):
    """sgc_precompute on a torch COO: T in, T out, the emulation's bits, for
    two feature sets; the fp32 call on the same adjacency afterwards still
    gives the reference's golden (no cache shared between the dtypes)."""
    from sgc_amd.utils import sgc_precompute
    c = tiny_cases["hub1000_F130"]
    n = int(c["n"])
    csr_h = oracle.coo_to_csr(n, n, c["rows"], c["cols"], c["vals"])
    idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64))
    adj = torch.sparse_coo_tensor(idx, torch.from_numpy(c["vals"]), (n, n)).to(DEV)
    X = torch.from_numpy(c["X"])
    for X16 in (X.to(dtype), torch.flip(X, dims=[0]).to(dtype)):
        out, secs = sgc_precompute(X16.to(DEV), adj, 2)
        assert out.dtype == dtype and out.device.type == "cuda" and secs > 0
        assert same_bits(out, emulate(oracle, csr_h, X16, 2))
    x16 = X.to(dtype).to(DEV)
    assert sgc_precompute(x16, adj, 0)[0] is x16
    out32, _ = sgc_precompute(X.to(DEV), adj, 2)
    assert out32.dtype == torch.float32
    assert np.array_equal(out32.cpu().numpy().view(np.uint32), c["Y2"].view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_unsupported_paths_raise(tiny_cases, dtype):
    from sgc_amd.propagate import DeviceCSR, GraphedPropagation, SpmmLaunch, propagate
    c = tiny_cases["norm_n48_F65"]
    n = int(c["n"])
    idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64))
    csr = DeviceCSR.from_torch(torch.sparse_coo_tensor(idx, torch.from_numpy(c["vals"]),
                                                       (n, n)).to(DEV))
    X = torch.from_numpy(c["X"]).to(dtype).to(DEV)
    with pytest.raises(TypeError, match="SpmmLaunch"):
        SpmmLaunch(csr, X, torch.empty_like(X))
    with pytest.raises(TypeError, match="native_loop"):
        propagate(csr, X, 2, native_loop=True)
    g = GraphedPropagation(csr, X.shape, 1)
    with pytest.raises(TypeError, match="GraphedPropagation"):
        g.run(X)
