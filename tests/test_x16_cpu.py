"""bfloat16 / float16 feature storage on CPU tensors and at the C ABI (no GPU).

Contract: 16 bits in memory, fp32 everywhere else.  Each hop is the fp32 path's
single sequential FMA chain on the exactly widened features, rounded to
nearest even once per stored element, so it equals -- with no tolerance --

    X_{k+1} = fp32_spmm(S, X_k.float()).to(T)

where fp32_spmm here is the oracle's restatement of torch.spmm's arithmetic.
"""
import numpy as np
import pytest
import torch

DTYPES = [torch.bfloat16, torch.float16]
CASES = ["norm_n48_F602", "norm_n48_F65", "raw_unsorted_dups_F7"]


@pytest.fixture(scope="module", autouse=True)
def _lib_built():
    from sgc_amd import build
    build.build(verbose=False)


def coo_cpu(c):
    n = int(c["n"])
    idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(c["vals"]), (n, n))


def bits16(t):
    return t.contiguous().view(torch.int16)


def emulate(oracle, csr, X16, K, last_fp32=False):
    """K hops of fp32_spmm(S, X.float()).to(T) (the last rounding dropped for
    last_fp32) with the oracle as fp32_spmm."""
    rp, ci, va = (np.ascontiguousarray(a) for a in csr)
    X = X16
    for h in range(K):
        Y = torch.from_numpy(oracle.spmm_csr(rp, ci, va, X.float().numpy(), 0, rp.size - 1))
        X = Y if (last_fp32 and h == K - 1) else Y.to(X16.dtype)
    return X


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_tiny_cases_cpu_bit_exact_x16(tiny_cases, oracle, name, dtype):
    from sgc_amd.utils import sgc_precompute
    c = tiny_cases[name]
    n = int(c["n"])
    csr = oracle.coo_to_csr(n, n, c["rows"], c["cols"], c["vals"])
    adj = coo_cpu(c)
    X = torch.from_numpy(c["X"]).to(dtype)
    out0, _ = sgc_precompute(X, adj, 0)
    assert out0 is X
    for K in (1, 2, 3):
        out, secs = sgc_precompute(X, adj, K)
        assert out.dtype == dtype and out.device.type == "cpu" and secs >= 0
        want = emulate(oracle, csr, X, K)
        assert torch.equal(bits16(out), bits16(want)), (name, K, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_fp32_output_and_spmm_x16(tiny_cases, oracle, dtype):
    """out_dtype=float32 drops the last rounding; spmm on a row range."""
    from sgc_amd.propagate import DeviceCSR, propagate, spmm
    c = tiny_cases["norm_n48_F65"]
    n = int(c["n"])
    csr = oracle.coo_to_csr(n, n, c["rows"], c["cols"], c["vals"])
    d = DeviceCSR.from_torch(coo_cpu(c))
    X = torch.from_numpy(c["X"]).to(dtype)
    out = propagate(d, X, 2, out_dtype=torch.float32)
    want = emulate(oracle, csr, X, 2, last_fp32=True)
    assert out.dtype == torch.float32
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    y = spmm(d, X, 5, 40)
    want1 = emulate(oracle, csr, X, 1)[5:40]
    assert y.dtype == dtype and torch.equal(bits16(y), bits16(want1))
    with pytest.raises(TypeError):
        propagate(d, X, 2, out_dtype=torch.float64)


@pytest.mark.parametrize("dtype,u", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_accuracy_bound_against_fp64(tiny_cases, dtype, u):
    """|X^_K - X_K| <= ((1 + u)^K - 1) . S^K |X_0| elementwise (S >= 0), X^ the
    16-bit run and X_K the exact product from the same X_0, here in fp64.
    The only slack is the fp32 roundoff of the chains themselves: a chain of
    d FMAs carries at most gamma_d = d eps / (1 - d eps) relative to S|X| per
    hop (eps = 2^-24, d = the longest row's nonzeros), so by induction over
    the hops |X^_K - X_K| <= (((1 + u)(1 + gamma_d))^K - 1) . S^K |X_0|: the
    bound above plus (1 + u)^K ((1 + gamma_d)^K - 1), about K d 2^-24."""
    from sgc_amd.utils import sgc_precompute
    c = tiny_cases["norm_n48_F65"]
    n = int(c["n"])
    assert (c["vals"] >= 0).all()
    adj = coo_cpu(c)
    S = adj.to_dense().double()
    X0 = torch.from_numpy(c["X"]).to(dtype)
    d_max = int(np.bincount(c["rows"].astype(np.int64), minlength=n).max())
    eps = 2.0 ** -24
    gamma = d_max * eps / (1 - d_max * eps)
    for K in (1, 2, 3):
        got, _ = sgc_precompute(X0, adj, K)
        exact, mag = X0.double(), X0.double().abs()
        for _ in range(K):
            exact, mag = S @ exact, S @ mag
        bound = (((1 + u) * (1 + gamma)) ** K - 1) * mag
        err = (got.double() - exact).abs()
        print(f"{dtype} K={K}: max err/bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (dtype, K)


def test_other_dtypes_still_raise():
    from sgc_amd.utils import sgc_precompute
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.tensor([1.0, 1.0]), (2, 2))
    for bad in (torch.float64, torch.int32, torch.int16):
        with pytest.raises(TypeError, match="features must be float32"):
            sgc_precompute(torch.zeros((2, 4), dtype=bad), adj, 1)
    with pytest.raises(TypeError):  # the adjacency stays fp32-only
        sgc_precompute(torch.zeros((2, 4), dtype=torch.bfloat16), adj.to(torch.bfloat16), 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_process_group_and_device_set_refuse_x16(monkeypatch, dtype):
    """Under an active process group (a stub here: the dispatch never reaches
    it) or SGC_AMD_DEVICES the partitioned paths are fp32-only."""
    from sgc_amd import multigpu, utils
    from sgc_amd.propagate import DeviceCSR
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.tensor([1.0, 1.0]), (2, 2))
    csr = DeviceCSR.from_torch(adj)
    X = torch.ones((2, 4), dtype=dtype)
    monkeypatch.setattr(multigpu, "process_group", lambda device: object())
    with pytest.raises(TypeError, match="process group"):
        utils._propagate_on_node(csr, X, 1)
    with pytest.raises(TypeError, match="process group"):
        utils.sgc_precompute(X, adj, 1)


def test_abi_x16_argument_checks():
    """Unknown dtypes and ACCUMULATE into a 16-bit Y are refused with a text;
    a valid combination stops at its null pointers, before touching a device
    (the pattern of test_spmm_ex_accepts_every_declared_flag)."""
    from sgc_amd import _lib
    lib = _lib.load()
    F32, BF16, F16 = 0, 1, 2
    ACCUMULATE = 16

    def call(xd, yd, flags):
        rc = lib.sgc_spmm_csr_x16(None, None, None, 0, 0, None, xd, 1, None, yd, 1, 1, None, 0, 0,
                                  0, flags, None)
        return rc, lib.sgc_last_error()

    for xd, yd in ((F32, F32), (3, 3), (-1, F32), (BF16, F16), (F16, BF16), (BF16, 7)):
        rc, msg = call(xd, yd, 0)
        assert rc != 0 and b"dtype" in msg, (xd, yd, msg)
    for xd in (BF16, F16):
        rc, msg = call(xd, xd, ACCUMULATE)
        assert rc != 0 and b"ACCUMULATE" in msg, msg
        rc, msg = call(xd, F32, ACCUMULATE)
        assert rc != 0 and b"null pointer" in msg, msg
        for yd in (xd, F32):
            for bit in (1, 2, 4, 8, 32, 64, 128):
                rc, msg = call(xd, yd, bit)
                assert rc != 0 and b"null pointer" in msg, (bit, msg)
        rc, msg = call(xd, xd, 256)
        assert rc != 0 and b"unknown flags" in msg
    assert lib.sgc_aligned_ld_x16(602) == 640 and lib.sgc_aligned_ld_x16(64) == 64
    assert lib.sgc_aligned_ld_x16(1) == 64 and lib.sgc_aligned_ld_x16(0) == 0
    assert lib.sgc_abi_version() == 1
