"""The ingest (csrc/ingest.hip), the radix sort behind it and behind
sgc_plan_sorted (csrc/sort.hip), and sgc_csr_to_coo64, on the device, at the
sizes where that code changes path: the cases of ingest_cases.py, which
test_ingest_cases_cpu.py shows would catch a one-line fault in the sort.

Everything is exact: integer arrays with np.array_equal, values by their
bit patterns, the status word against the numpy rule.  Every output buffer is
a few elements longer than it need be and pre-filled; the slack must keep its
fill (no write past an array).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ingest_cases as ic

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLACK = 5
FILL32, FILL64 = -0x21524111, -0x2152411021524111     # in no expected array
SGC_OK, SGC_EINVAL, SGC_ERANGE, SGC_ENOMEM = 0, 1, 2, 4


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(Coo, Ref) of a case: computed once, shared, read-only."""
    case = ic.coo_case(name)
    ref = ic.reference(*case)
    for a in (*case[:3], *ref[:3]):
        a.setflags(write=False)
    return case, ref


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # (a copy: the cases are read-only)


def filled(n, dtype=torch.int32):
    return torch.full((n + SLACK,), FILL64 if dtype == torch.int64 else FILL32, dtype=dtype,
                      device=DEV)


def take(buf, n):
    """The first n elements of an output buffer, on the host; the slack after
    them must be untouched."""
    a = buf.cpu().numpy()
    fill = FILL64 if a.dtype == np.int64 else FILL32
    assert (a[n:] == fill).all(), "a write past the end of an output array"
    return a[:n]


def lib_and_stream():
    from sgc_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream_handle(DEV)


def raw_coo_to_csr(case, with_status=True, sizes=None, ws_short=0):
    """sgc_coo_to_csr through the raw ABI, the workspace sized by
    sgc_coo_to_csr_workspace: (return code, status, (row_ptr, col, val))."""
    lib, ptr, stream = lib_and_stream()
    nnz = len(case.rows)
    rows, cols, vals = dev(case.rows), dev(case.cols), dev(case.vals)
    row_ptr, col, val = filled(case.n_rows + 1), filled(nnz), filled(nnz)   # val: fp32 bits
    need = ctypes.c_size_t(0)
    assert lib.sgc_coo_to_csr_workspace(case.n_rows, nnz, ctypes.byref(need)) == SGC_OK
    ws = torch.empty(max(1, need.value), dtype=torch.uint8, device=DEV)
    status = ctypes.c_uint32(0xffffffff)
    a_nnz, a_rows, a_cols = sizes or (nnz, case.n_rows, case.n_cols)
    rc = lib.sgc_coo_to_csr(ptr(rows), ptr(cols), ptr(vals), a_nnz, a_rows, a_cols, ptr(row_ptr),
                            ptr(col), ptr(val), ptr(ws), need.value - ws_short,
                            ctypes.byref(status) if with_status else None, stream)
    torch.cuda.synchronize()
    got = (take(row_ptr, case.n_rows + 1), take(col, nnz), take(val, nnz).view(np.float32))
    return rc, status.value, got


def raw_csr64_to_csr(crow, col64, vals, n_cols, with_status=True, sizes=None):
    lib, ptr, stream = lib_and_stream()
    n_rows, nnz = len(crow) - 1, len(col64)
    crow_d, col_d, val_d = dev(np.asarray(crow, np.int64)), dev(np.asarray(col64, np.int64)), dev(vals)
    row_ptr, col, val = filled(n_rows + 1), filled(nnz), filled(nnz)
    status = ctypes.c_uint32(0xffffffff)
    a_nnz, a_rows, a_cols = sizes or (nnz, n_rows, n_cols)
    rc = lib.sgc_csr64_to_csr(ptr(crow_d), ptr(col_d), ptr(val_d), a_nnz, a_rows, a_cols,
                              ptr(row_ptr), ptr(col), ptr(val),
                              ctypes.byref(status) if with_status else None, stream)
    torch.cuda.synchronize()
    got = (take(row_ptr, n_rows + 1), take(col, nnz), take(val, nnz).view(np.float32))
    return rc, status.value, got


def assert_csr(got, ref, what):
    rp, ci, va = (a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in got)
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and va.dtype == np.float32, what
    assert np.array_equal(rp, ref.row_ptr), f"{what}: row_ptr"
    assert np.array_equal(ci, ref.col), f"{what}: col_idx"
    assert np.array_equal(ic.bits(va), ic.bits(ref.val)), f"{what}: value bits"


def coo_tensor(case):
    idx = torch.from_numpy(np.stack([case.rows, case.cols]).reshape(2, -1))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.array(case.vals)),
                                   (case.n_rows, case.n_cols), check_invariants=False).to(DEV)


def last_error():
    return lib_and_stream()[0].sgc_last_error()


# ---------------------------------------------------------------------------
# COO ingest

@pytest.mark.parametrize("name", list(ic.COO_CASES))
def test_raw_coo_ingest_equals_reference(name):
    case, ref = case_and_ref(name)
    rc, status, got = raw_coo_to_csr(case)
    assert rc == SGC_OK, last_error()
    assert_csr(got, ref, name)
    assert status == ref.status, f"{name}: status {status}, the reference has {ref.status}"
    assert status == ic.EXPECTED_STATUS.get(name, status)


@pytest.mark.parametrize("name", list(ic.SMALL_CASES))
def test_from_torch_coo_ingest_equals_reference(name):
    from sgc_amd.propagate import DeviceCSR
    case, ref = case_and_ref(name)
    csr = DeviceCSR.from_torch(coo_tensor(case))
    assert (csr.n_rows, csr.n_cols, csr.nnz) == (case.n_rows, case.n_cols, len(case.rows))
    assert_csr((csr.row_ptr, csr.col_idx, csr.val), ref, name)
    assert csr.status == ref.status
    if name.startswith("column_major"):
        # a column-major COO keeps the column groups: the bit describes the CSR
        assert csr.cols_ascending and csr.status == 2
        groups = csr.column_groups(2)
        assert len(groups) == 2 and all(g.row_ptr.numel() == case.n_rows + 1 for g in groups)


def test_one_hop_on_the_scan_carry_csr_equals_the_oracle(oracle):
    """4.2 million unsorted entries with a hub row through from_torch (1,025
    scan blocks), then one hop at F = 3 against the oracle on the reference
    CSR.  Ordinary random values here: with them the FMA order shows."""
    from sgc_amd.propagate import DeviceCSR, spmm
    case, _ = case_and_ref("scan_carry")
    rng = np.random.default_rng(20)
    case = case._replace(vals=rng.standard_normal(len(case.rows)).astype(np.float32))
    ref = ic.reference(*case)
    csr = DeviceCSR.from_torch(coo_tensor(case))
    assert_csr((csr.row_ptr, csr.col_idx, csr.val), ref, "scan_carry")
    assert csr.status == ref.status
    X = rng.standard_normal((case.n_cols, 3)).astype(np.float32)
    y = spmm(csr, torch.from_numpy(X).to(DEV)).cpu().numpy()
    want = oracle.spmm_csr(ref.row_ptr, ref.col, ref.val, X)
    assert y.shape == want.shape and np.array_equal(ic.bits(y), ic.bits(want))


@pytest.mark.parametrize("name", list(ic.PLAN_CASES))
def test_plan_sorted_past_the_scan_carry(name):
    """sgc_plan_sorted over 2048 x 2048 + 3 rows (descending, two passes, a
    carried block-sum scan; last_bin: with slots that come from the carried
    block) and over three tiles: longest first, ties in row order, and the
    three counts."""
    lib, ptr, stream = lib_and_stream()
    deg = ic.PLAN_CASES[name]()
    n = len(deg)
    rp = np.concatenate([[0], np.cumsum(deg)])
    assert rp[-1] < 2 ** 31
    rp_d = dev(rp.astype(np.int32))
    out = filled(n)
    wb = lib.sgc_plan_sorted_workspace(n)
    ws = torch.empty(max(1, wb), dtype=torch.uint8, device=DEV)
    counts = (ctypes.c_int64 * 3)()
    rc = lib.sgc_plan_sorted(ptr(rp_d), 0, n, 64, 1024, ptr(out), ptr(ws), wb,
                             ctypes.cast(counts, ctypes.c_void_p), stream)
    assert rc == SGC_OK, last_error()
    torch.cuda.synchronize()
    assert list(counts) == [int((deg > 64).sum()), int((deg > 1024).sum()), int(deg.max())]
    assert np.array_equal(take(out, n), np.argsort(-deg, kind="stable").astype(np.int32))


# ---------------------------------------------------------------------------
# inputs the ingest must refuse

@pytest.mark.parametrize("name", list(ic.narrowing()))
def test_coo_ingest_refuses_indices_that_only_fit_once_narrowed(name):
    from sgc_amd._lib import SGCError
    from sgc_amd.propagate import DeviceCSR
    case = ic.narrowing()[name]
    rc, status, _ = raw_coo_to_csr(case)
    assert rc == SGC_ERANGE and status & ic.OUT_OF_RANGE
    assert last_error()
    assert raw_coo_to_csr(case, with_status=False)[0] == SGC_ERANGE
    with pytest.raises(SGCError):
        DeviceCSR.from_torch(coo_tensor(case))


@pytest.mark.parametrize("name", list(ic.bad_crow()))
def test_csr_ingest_refuses_a_bad_layout(name):
    """crow must be a layout of the nnz entries: 0 first, nnz last, never
    decreasing, inside [0, nnz]; columns inside [0, n_cols)."""
    from sgc_amd._lib import SGCError
    from sgc_amd.propagate import DeviceCSR
    crow, col, vals = ic.bad_crow()[name]
    rc, status, _ = raw_csr64_to_csr(crow, col, vals, ic.BAD_CROW_SHAPE[1])
    assert rc == SGC_ERANGE and status & ic.OUT_OF_RANGE, f"{name}: code {rc}, status {status}"
    assert last_error()
    assert raw_csr64_to_csr(crow, col, vals, ic.BAD_CROW_SHAPE[1], with_status=False)[0] == SGC_ERANGE
    adj = torch.sparse_csr_tensor(dev(crow), dev(col), dev(vals), ic.BAD_CROW_SHAPE,
                                  check_invariants=False)
    with pytest.raises(SGCError):
        DeviceCSR.from_torch(adj)


def test_csr_ingest_takes_the_valid_small_layout():
    crow, col, vals = ic.valid_small_csr()
    rc, status, got = raw_csr64_to_csr(crow, col, vals, ic.BAD_CROW_SHAPE[1])
    assert rc == SGC_OK and status == 3
    assert_csr(got, ic.reference_csr(crow, col, vals, ic.BAD_CROW_SHAPE[1]), "valid")


# ---------------------------------------------------------------------------
# CSR ingest

def _csr_variants():
    out = {}
    for name in ("sorted_gaps[10000]", "sorted_gaps[1]", "sorted_gaps[0]",
                 "column_major[400x300]", "column_major[300x400]"):
        out[name] = (name, None)
    out["column_major,one_row_reversed"] = ("column_major[400x300]", "reverse")
    out["column_major,one_duplicated_column"] = ("column_major[400x300]", "duplicate")
    return out


@pytest.mark.parametrize("variant", list(_csr_variants()))
def test_csr_ingest_equals_reference(variant):
    name, change = _csr_variants()[variant]
    case, ref = case_and_ref(name)
    crow, col, vals = ref.row_ptr.astype(np.int64), ref.col.astype(np.int64), ref.val
    if change:
        col = col.copy()
        row = int(np.flatnonzero(np.diff(crow) >= 3)[7])
        lo, hi = crow[row], crow[row + 1]
        if change == "reverse":
            col[lo:hi] = col[lo:hi][::-1].copy()
        else:
            col[lo + 1] = col[lo]
    want = ic.reference_csr(crow, col, vals, case.n_cols)
    assert want.status == (1 if change else 3)
    rc, status, got = raw_csr64_to_csr(crow, col, vals, case.n_cols)
    assert rc == SGC_OK, last_error()
    assert_csr(got, want, variant)
    assert status == want.status, f"{variant}: status {status}, the reference has {want.status}"
    assert raw_csr64_to_csr(crow, col, vals, case.n_cols, with_status=False)[0] == SGC_OK


# ---------------------------------------------------------------------------
# sgc_csr_to_coo64

COO64_GRID_ROWS = 16384 * 256         # one pass of normalize.hip's largest grid


def _coo64_layouts():
    def wrap():
        deg = np.zeros(COO64_GRID_ROWS + 300, np.int64)
        at = [0, 5, COO64_GRID_ROWS - 1, COO64_GRID_ROWS, COO64_GRID_ROWS + 7, COO64_GRID_ROWS + 299]
        deg[at] = [3, 1, 2, 4, 70, 5]
        return deg
    return {
        "hub_row_next_to_empty_rows": lambda: np.array([0, 0, 50000, 0, 2, 0], np.int64),
        "sorted_gaps": lambda: np.diff(case_and_ref("sorted_gaps[10000]")[1].row_ptr).astype(np.int64),
        "no_rows": lambda: np.zeros(0, np.int64),
        "more_rows_than_one_grid_pass": wrap,
    }


@pytest.mark.parametrize("layout", list(_coo64_layouts()))
def test_csr_to_coo64(layout):
    lib, ptr, stream = lib_and_stream()
    deg = _coo64_layouts()[layout]()
    n = len(deg)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    col = np.random.default_rng(21).integers(0, 2 ** 31 - 1, nnz).astype(np.int32)
    rows64, cols64 = filled(nnz, torch.int64), filled(nnz, torch.int64)
    row_ptr_d, col_d = dev(row_ptr), dev(col)
    rc = lib.sgc_csr_to_coo64(ptr(row_ptr_d), ptr(col_d), n, ptr(rows64), ptr(cols64), stream)
    assert rc == SGC_OK, last_error()
    torch.cuda.synchronize()
    assert np.array_equal(take(rows64, nnz), np.repeat(np.arange(n, dtype=np.int64), deg))
    assert np.array_equal(take(cols64, nnz), col.astype(np.int64))


@pytest.mark.parametrize("name", ["sorted_gaps[10000]", "column_major[400x300]", "special_value_bits"])
def test_to_torch_coo_round_trip(name):
    """DeviceCSR -> to_torch_coo -> from_torch, the attached cache removed so
    that it really ingests again: the same three arrays; the status too,
    with bit 1 added where the first input was not row-sorted (the COO of a
    CSR is)."""
    from sgc_amd.propagate import DeviceCSR, to_torch_coo
    case, ref = case_and_ref(name)
    csr = DeviceCSR.from_torch(coo_tensor(case))
    adj = to_torch_coo(csr)
    if hasattr(adj, "_sgc_amd_csr"):
        del adj._sgc_amd_csr
    idx = adj._indices().cpu().numpy()
    assert idx.dtype == np.int64 and idx.shape == (2, csr.nnz)
    assert np.array_equal(idx[0], np.repeat(np.arange(case.n_rows), np.diff(ref.row_ptr)))
    assert np.array_equal(idx[1], ref.col)
    back = DeviceCSR.from_torch(adj)
    assert back is not csr
    assert_csr((back.row_ptr, back.col_idx, back.val), ref, name)
    assert back.status == csr.status | ic.ROWS_SORTED == ref.status | ic.ROWS_SORTED


# ---------------------------------------------------------------------------
# the raw ABI's error returns (each returns before any launch or pointer use:
# the size checks open coo_to_csr / csr64_to_csr / csr_to_coo64, the workspace
# check follows the layout arithmetic)

def test_coo_ingest_error_returns():
    lib, ptr, stream = lib_and_stream()
    case, ref = case_and_ref("nnz_edges[65]")
    nnz, big = len(case.rows), 2 ** 31 - 1
    assert raw_coo_to_csr(case, ws_short=1)[0] == SGC_ENOMEM and b"workspace" in last_error()
    for sizes in ((big, case.n_rows, case.n_cols), (nnz, big, case.n_cols), (nnz, case.n_rows, big)):
        assert raw_coo_to_csr(case, sizes=sizes)[0] == SGC_ERANGE and last_error(), sizes
    for sizes in ((-1, case.n_rows, case.n_cols), (nnz, -1, case.n_cols), (nnz, case.n_rows, -1)):
        assert raw_coo_to_csr(case, sizes=sizes)[0] == SGC_EINVAL and last_error(), sizes
    need = ctypes.c_size_t(0)
    assert lib.sgc_coo_to_csr_workspace(big, 10, ctypes.byref(need)) == SGC_ERANGE and last_error()
    assert lib.sgc_coo_to_csr_workspace(10, big, ctypes.byref(need)) == SGC_ERANGE
    assert lib.sgc_coo_to_csr_workspace(-1, 10, ctypes.byref(need)) == SGC_ERANGE
    assert lib.sgc_coo_to_csr_workspace(10, 10, None) == SGC_EINVAL and last_error()
    # status_host = NULL: the same arrays
    rc, _, got = raw_coo_to_csr(case, with_status=False)
    assert rc == SGC_OK
    assert_csr(got, ref, "status_host NULL")


def test_csr_ingest_and_coo64_error_returns():
    lib, ptr, stream = lib_and_stream()
    crow, col, vals = ic.valid_small_csr()
    n_rows, n_cols = ic.BAD_CROW_SHAPE
    nnz, big = len(col), 2 ** 31 - 1
    for sizes in ((big, n_rows, n_cols), (nnz, big, n_cols), (nnz, n_rows, big)):
        assert raw_csr64_to_csr(crow, col, vals, n_cols, sizes=sizes)[0] == SGC_ERANGE, sizes
        assert last_error()
    for sizes in ((-1, n_rows, n_cols), (nnz, -1, n_cols), (nnz, n_rows, -1)):
        assert raw_csr64_to_csr(crow, col, vals, n_cols, sizes=sizes)[0] == SGC_EINVAL, sizes
        assert last_error()
    rows64, cols64 = filled(nnz, torch.int64), filled(nnz, torch.int64)
    rp, ci = dev(crow.astype(np.int32)), dev(col.astype(np.int32))
    assert lib.sgc_csr_to_coo64(ptr(rp), ptr(ci), -1, ptr(rows64), ptr(cols64), stream) == SGC_EINVAL
    assert last_error()
    assert lib.sgc_csr_to_coo64(None, ptr(ci), n_rows, ptr(rows64), ptr(cols64), stream) == SGC_EINVAL
    torch.cuda.synchronize()
    take(rows64, 0), take(cols64, 0)        # nothing written at all
