"""Graph construction on the device -- AugNorm, induced sub-graph, COO/CSR
ingest -- at the edges binary symmetric graphs never reach.

The expected S of every case in graph_edge_cases.py is what the reference
itself returned (tests/golden/graph_edges.npz, made by gen_graph_edges.py);
the comparison rule is graph_edge_cases.compare_s: the reference's entries,
NaN where it has NaN, its fp32 bits everywhere else.  The sub-graph is held
to scipy's slice, the ingest to a stable numpy sort by row.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graph_edge_cases as g

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_edges.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_case(golden, name):
    n = len(golden[f"{name}/indptr"]) - 1
    A = g.from_arrays(n, golden[f"{name}/indptr"], golden[f"{name}/indices"], golden[f"{name}/data"])
    return A, tuple(golden[f"{name}/{k}"] for k in ("row", "col", "val"))


def csr_coo_host(csr):
    rp = csr.row_ptr.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(csr.n_rows, dtype=np.int64), np.diff(rp))
    return rows, csr.col_idx.cpu().numpy().astype(np.int64), csr.val.cpu().numpy()


def check_device_csr(csr, n, want, what):
    want_row, want_col, want_val = want
    rp = csr.row_ptr.cpu().numpy()
    assert csr.n_rows == n and csr.n_cols == n and rp.shape == (n + 1,), what
    assert csr.nnz == len(want_row), f"{what}: nnz {csr.nnz}, the reference has {len(want_row)}"
    assert csr.col_idx.numel() == csr.nnz and csr.val.numel() == csr.nnz, what
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(want_row, minlength=n))])
    assert np.array_equal(rp, want_ptr), f"{what}: row_ptr"
    g.compare_s(*csr_coo_host(csr), want_row, want_col, want_val, what=what)


# ---------------------------------------------------------------------------
# AugNorm

@pytest.mark.parametrize("name", g.CASE_NAMES)
def test_device_augnorm_matches_reference(golden, name):
    from sgc_amd.normalization import aug_normalize_on_device
    A, want = golden_case(golden, name)
    check_device_csr(aug_normalize_on_device(A), A.shape[0], want, name)


@pytest.mark.parametrize("name", g.CASE_NAMES)
def test_loader_coo_has_reference_indices_and_values(golden, name):
    from sgc_amd.normalization import aug_normalize_on_device
    from sgc_amd.propagate import to_torch_coo
    A, (row, col, val) = golden_case(golden, name)
    adj = to_torch_coo(aug_normalize_on_device(A))
    assert adj.is_sparse and adj.dtype == torch.float32 and tuple(adj.shape) == A.shape
    # the flag of the tensor the reference builds from the same S (torch calls
    # fewer than two entries coalesced, anything else as constructed is not)
    ref = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.from_numpy(val),
                                  A.shape)
    assert adj.is_coalesced() == ref.is_coalesced() and (len(row) < 2 or not adj.is_coalesced())
    idx = adj._indices().cpu().numpy()
    assert idx.dtype == np.int64 and idx.shape == (2, len(row))
    g.compare_s(idx[0], idx[1], adj._values().cpu().numpy(), row, col, val, what=name)


@pytest.mark.parametrize("name", g.PROPAGATION_CASES)
def test_one_hop_on_device_s_equals_spmm_on_reference_s(golden, name):
    from sgc_amd.normalization import aug_normalize_on_device
    from sgc_amd.propagate import to_torch_coo
    from sgc_amd.utils import sgc_precompute
    A, (row, col, val) = golden_case(golden, name)
    n = A.shape[0]
    X = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 19)).astype(np.float32))
    S_ref = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.from_numpy(val),
                                    (n, n))
    want = torch.spmm(S_ref, X).numpy()
    out, _ = sgc_precompute(X.to(DEV), to_torch_coo(aug_normalize_on_device(A)), 1)
    got = out.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), name
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), name


def test_device_augnorm_grid_stride_wraps():
    """More rows than one pass of the largest grid (16384 blocks of 256): a
    weighted ring, CSR built directly.  Every row sum is a small integer, so
    the expected S is exact in any order and is computed vectorised."""
    from sgc_amd.normalization import aug_normalize_device_arrays
    n = 16384 * 256 + 300
    i = np.arange(n, dtype=np.int32)
    w = 1.0 + (i % 3)                                       # a_ij = 1 + j mod 3
    prev, nxt = lambda x: np.roll(x, 1), lambda x: np.roll(x, -1)   # x[i-1], x[i+1] on the ring
    d = np.power(1.0 + prev(w) + nxt(w), -0.5)              # sums in 3..6, exact
    # A: row i = {i-1, i+1}; S: row i = {i-1, i, i+1}; rows 0 and n-1 wrap, so
    # their columns ascend in another order
    indices = np.stack([prev(i), nxt(i)], axis=1)
    data = np.stack([prev(w), nxt(w)], axis=1)
    cols = np.stack([prev(i), i, nxt(i)], axis=1)
    want = np.stack([(d * prev(w)) * prev(d), (d * 1.0) * d, (d * nxt(w)) * nxt(d)], axis=1)
    indices[0], data[0] = indices[0, ::-1].copy(), data[0, ::-1].copy()
    indices[-1], data[-1] = indices[-1, ::-1].copy(), data[-1, ::-1].copy()
    cols[0], want[0] = cols[0, [1, 2, 0]], want[0, [1, 2, 0]]
    cols[-1], want[-1] = cols[-1, [2, 0, 1]], want[-1, [2, 0, 1]]
    assert (np.diff(indices, axis=1) > 0).all() and (np.diff(cols, axis=1) > 0).all()
    indptr = (2 * np.arange(n + 1)).astype(np.int32)
    want_val = want.astype(np.float32).ravel()
    got = aug_normalize_device_arrays(torch.from_numpy(indptr).to(DEV),
                                      torch.from_numpy(indices.ravel()).to(DEV),
                                      torch.from_numpy(data.ravel()).to(DEV), n)
    assert got.nnz == 3 * n
    assert torch.equal(got.row_ptr, torch.arange(0, 3 * n + 1, 3, dtype=torch.int32, device=DEV))
    assert torch.equal(got.col_idx, torch.from_numpy(cols.ravel().astype(np.int32)).to(DEV))
    assert torch.equal(got.val.view(torch.int32),
                       torch.from_numpy(want_val.view(np.int32)).to(DEV))


# ---------------------------------------------------------------------------
# induced sub-graph

def _sub_host(A, idx):
    """The reference's slice (utils.py:117), canonicalised."""
    B = sp.csr_matrix(A[idx, :][:, idx])
    B.sum_duplicates()
    B.sort_indices()
    return B


def check_subgraph(A, idx):
    from sgc_amd.normalization import device_csr64, subgraph_on_device
    rp, ci, va, m = subgraph_on_device(*device_csr64(A), idx)
    want = _sub_host(A, idx)
    assert m == len(idx)
    assert np.array_equal(rp.cpu().numpy(), want.indptr)
    assert np.array_equal(ci.cpu().numpy(), want.indices)
    assert np.array_equal(va.cpu().numpy().view(np.uint64), want.data.view(np.uint64))
    return want


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_device_subgraph_keep_patterns(order):
    """Rows of 0, 1, 63, 64, 65, 128, 129 and 1000 entries whose 64-entry
    chunks keep none, all, every other, only lane 0, only lane 63 and a run
    across a chunk edge; stored zeros, NaN and inf among the values."""
    A, kept = g.subgraph_source()
    idx = {"ascending": kept, "descending": kept[::-1].copy(),
           "shuffled": np.random.default_rng(6).permutation(kept)}[order]
    want = check_subgraph(A, idx)
    assert (want.data == 0).any() and np.isnan(want.data).any() and np.isinf(want.data).any()
    long_row = int(np.nonzero(idx == g.SUB_FIRST_ROW + len(g.SUB_ROW_LENGTHS) - 1)[0][0])
    assert np.diff(want.indptr)[long_row] > 300      # the long row keeps several chunks' worth


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_device_subgraph_sort_key_bits(m):
    """m on both sides of a power of two: the segmented sort's key bits."""
    A, _ = g.subgraph_source()
    want = check_subgraph(A, g.subgraph_small_index(m))
    assert m < 63 or want.nnz > m


def test_device_subgraph_stride_wraps():
    """m = 70,000 rows of a sparse 80,000-node graph: the wave-per-row count
    and fill kernels' stride loops wrap above 65,536 rows."""
    rng = np.random.default_rng(12)
    n, m = 80000, 70000
    r, c = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    A = sp.coo_matrix((rng.standard_normal(3 * n), (r, c)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    check_subgraph(A, rng.permutation(n)[:m])


def test_device_subgraph_then_augnorm_matches_reference(golden):
    from sgc_amd.normalization import aug_normalize_device_arrays, device_csr64, subgraph_on_device
    A, _ = golden_case(golden, g.SUBGRAPH_CASE)
    idx = golden["sub/idx"]
    got = aug_normalize_device_arrays(*subgraph_on_device(*device_csr64(A), idx))
    check_device_csr(got, len(idx), (golden["sub/row"], golden["sub/col"], golden["sub/val"]),
                     "sub")


# ---------------------------------------------------------------------------
# ingest

def _coo(rows, cols, shape, vals=None):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if vals is None:      # distinct values: a misplaced entry cannot hide
        vals = (np.arange(len(rows)) + 1).astype(np.float32)
    idx = torch.from_numpy(np.stack([rows, cols]).reshape(2, -1))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(vals, np.float32)), shape,
                                   check_invariants=False).to(DEV)


def check_coo_ingest(rows, cols, shape):
    from sgc_amd.propagate import STATUS_COLS_ASCENDING, STATUS_ROWS_SORTED, DeviceCSR
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = (np.arange(len(rows)) + 1).astype(np.float32)
    csr = DeviceCSR.from_torch(_coo(rows, cols, shape, vals))
    order = np.argsort(rows, kind="stable")
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=shape[0]))])
    assert (csr.n_rows, csr.n_cols) == tuple(shape) and csr.nnz == len(rows)
    assert np.array_equal(csr.row_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(csr.col_idx.cpu().numpy(), cols[order])
    assert np.array_equal(csr.val.cpu().numpy(), vals[order])
    rows_sorted = bool(np.all(np.diff(rows) >= 0))
    same_row = np.diff(rows[order]) == 0
    ascending = bool(np.all(np.diff(cols[order])[same_row] > 0))
    assert bool(csr.status & STATUS_ROWS_SORTED) == rows_sorted
    assert bool(csr.status & STATUS_COLS_ASCENDING) == ascending   # of the CSR, sorted input or not
    assert not csr.status & 4
    return csr


COO_CASES = {
    "no_entries": ([], [], (5, 5)),
    "one_entry": ([3], [1], (6, 4)),
    "one_entry_last_corner": ([5], [3], (6, 4)),
    "all_in_one_row": ([2] * 7, [0, 1, 2, 3, 4, 5, 6], (5, 7)),
    "all_in_one_row_unordered_columns": ([2] * 7, [3, 1, 6, 0, 5, 2, 4], (5, 7)),
    "empty_rows_around_sorted": ([3, 3, 4, 6], [0, 2, 1, 5], (10, 6)),
    "empty_rows_around_unsorted": ([6, 3, 4, 3], [5, 0, 1, 2], (10, 6)),
    "adjacent_equal_pairs": ([0, 1, 1, 1, 2], [0, 2, 2, 3, 1], (3, 4)),
    "sorted_rows_descending_columns": ([0, 0, 0, 1, 1, 2], [3, 2, 0, 3, 1, 2], (3, 4)),
    "unsorted_rows_ascending_columns": ([2, 0, 2, 0, 1], [0, 1, 3, 2, 1], (3, 4)),
}


@pytest.mark.parametrize("name", list(COO_CASES))
def test_coo_ingest_matches_stable_row_sort(name):
    from sgc_amd.propagate import STATUS_COLS_ASCENDING, STATUS_ROWS_SORTED
    rows, cols, shape = COO_CASES[name]
    csr = check_coo_ingest(rows, cols, shape)
    if name == "adjacent_equal_pairs":
        assert csr.status & STATUS_ROWS_SORTED and not csr.status & STATUS_COLS_ASCENDING
    if name == "sorted_rows_descending_columns":
        assert csr.status & STATUS_ROWS_SORTED and not csr.status & STATUS_COLS_ASCENDING


@pytest.mark.parametrize("rows,cols", [([0, -1, 2], [0, 1, 2]), ([0, 3, 2], [0, 1, 2]),
                                       ([0, 1, 2], [0, -1, 2]), ([0, 1, 2], [0, 4, 2])],
                         ids=["row<0", "row>=n_rows", "col<0", "col>=n_cols"])
def test_coo_ingest_rejects_out_of_range(rows, cols):
    from sgc_amd._lib import SGCError
    from sgc_amd.propagate import DeviceCSR
    with pytest.raises(SGCError):
        DeviceCSR.from_torch(_coo(rows, cols, (3, 4)))


def _csr_tensor(crow, col, shape):
    vals = (np.arange(len(col)) + 1).astype(np.float32)
    t = torch.sparse_csr_tensor(torch.tensor(crow, dtype=torch.int64, device=DEV),
                                torch.tensor(col, dtype=torch.int64, device=DEV),
                                torch.from_numpy(vals).to(DEV), shape, check_invariants=False)
    return t, vals


@pytest.mark.parametrize("name,crow,col,ascending", [
    ("empty_first_last_rows", [0, 0, 2, 3, 3], [1, 4, 0], True),
    ("unsorted_columns", [0, 0, 3, 4, 4], [4, 1, 2, 0], False),
    ("duplicate_columns", [0, 0, 3, 4, 4], [1, 1, 2, 0], False),
    ("no_entries", [0, 0, 0, 0, 0], [], True),
])
def test_csr_ingest_keeps_layout_and_reports_columns(name, crow, col, ascending):
    from sgc_amd.propagate import STATUS_COLS_ASCENDING, STATUS_ROWS_SORTED, DeviceCSR
    adj, vals = _csr_tensor(crow, col, (4, 5))
    csr = DeviceCSR.from_torch(adj)
    assert (csr.n_rows, csr.n_cols, csr.nnz) == (4, 5, len(col))
    assert csr.row_ptr.dtype == torch.int32 and csr.col_idx.dtype == torch.int32
    assert np.array_equal(csr.row_ptr.cpu().numpy(), np.asarray(crow))
    assert np.array_equal(csr.col_idx.cpu().numpy(), np.asarray(col, np.int32))
    assert np.array_equal(csr.val.cpu().numpy(), vals)
    assert csr.status & STATUS_ROWS_SORTED
    assert bool(csr.status & STATUS_COLS_ASCENDING) == ascending


@pytest.mark.parametrize("bad", [-1, 5], ids=["col<0", "col>=n_cols"])
def test_csr_ingest_rejects_out_of_range_column(bad):
    from sgc_amd._lib import SGCError
    from sgc_amd.propagate import DeviceCSR
    adj, _ = _csr_tensor([0, 0, 2, 3, 3], [1, bad, 0], (4, 5))
    with pytest.raises(SGCError):
        DeviceCSR.from_torch(adj)
