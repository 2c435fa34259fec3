"""Small adjacencies that take graph construction through its edges.

S = D^-1/2 (A+I) D^-1/2 is the operand of every later result.  On binary
symmetric graphs every row sum is a positive integer, every d is an ordinary
number and nothing is ever pruned, so several kinds of error change nothing
there: a wrong drop rule, a row sum taken in another order or precision, a
diagonal inserted at the wrong place, stored zeros counted.  The graphs built
here make each of them visible; what the reference makes of them is recorded
in tests/golden/graph_edges.npz (tests/golden/gen_graph_edges.py).

cases()            {name: canonical scipy CSR, fp64 values}, each the smallest
                   that reaches its branch (stored zeros are kept as entries)
SUBGRAPH_CASE/idx  the signed case and index set of the slice-then-normalise test
aplus_i_row        row i of A+I as the reference forms it (diagonal at its
                   sorted position, exact zeros pruned)
sequential_sum     the reference's fp64 row sum: left to right from +0.0
compare_s          the one comparison rule: same entries, NaN where the
                   reference is NaN (payload and sign free), equal fp32 bits
                   everywhere else
subgraph_source    the graph, index sets and patterns of the sub-graph tests

Plain numpy + scipy; no GPU, no native library, no pytest.
"""
import functools

import numpy as np
import scipy.sparse as sp

INF, NAN = np.inf, np.nan
BIG = 2.0 ** 53          # BIG + 1 == BIG in fp64 (ties to even)
BIG32 = 2.0 ** 30        # BIG32 + 1 == BIG32 in fp32 only


def from_entries(n, entries):
    """Canonical CSR from {(i, j): value}; every entry stays stored, zeros too."""
    keys = sorted(entries)
    rows = np.array([k[0] for k in keys], np.int64)
    indices = np.array([k[1] for k in keys], np.int32)
    data = np.array([entries[k] for k in keys], np.float64)
    indptr = np.zeros(n + 1, np.int32)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr).astype(np.int32)
    return from_arrays(n, indptr, indices, data)


def from_arrays(n, indptr, indices, data):
    A = sp.csr_matrix((np.asarray(data, np.float64), np.asarray(indices, np.int32),
                       np.asarray(indptr, np.int32)), shape=(n, n))
    assert A.has_canonical_format
    return A


def aplus_i_row(A, i, diagonal="sorted", stored_zeros=False):
    """(columns, values) of row i of A+I.  diagonal="sorted" is the reference
    (inserted at its sorted position when absent); "last" appends an absent
    one.  stored_zeros=True keeps a stored +-0.0 of A as an entry."""
    cols = A.indices[A.indptr[i]:A.indptr[i + 1]].astype(np.int64)
    vals = A.data[A.indptr[i]:A.indptr[i + 1]].astype(np.float64)
    hit = np.nonzero(cols == i)[0]
    if hit.size:
        vals = vals.copy()
        with np.errstate(invalid="ignore"):
            vals[hit[0]] = vals[hit[0]] + 1.0
        keep = vals != 0.0
        if stored_zeros:
            keep |= cols != i
    else:
        keep = vals != 0.0
        if stored_zeros:
            keep[:] = True
        at = int(np.searchsorted(cols, i)) if diagonal == "sorted" else len(cols)
        cols = np.insert(cols, at, i)
        vals = np.insert(vals, at, 1.0)
        keep = np.insert(keep, at, True)
    return cols[keep], vals[keep]


def sequential_sum(vals, dtype=np.float64):
    acc = dtype(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in np.asarray(vals, dtype):
            acc = dtype(acc + v)
    return acc


def compare_s(got_row, got_col, got_val, want_row, want_col, want_val, what=""):
    got_val = np.asarray(got_val)
    want_val = np.asarray(want_val)
    assert got_val.dtype == np.float32 and want_val.dtype == np.float32, what
    assert len(got_row) == len(want_row), \
        f"{what}: {len(got_row)} entries, the reference has {len(want_row)}"
    assert np.array_equal(got_row, want_row) and np.array_equal(got_col, want_col), \
        f"{what}: entries at other positions than the reference's"
    nan = np.isnan(want_val)
    assert np.array_equal(np.isnan(got_val), nan), f"{what}: NaN entries differ"
    assert np.array_equal(got_val.view(np.uint32)[~nan], want_val.view(np.uint32)[~nan]), \
        f"{what}: values differ from the reference's fp32 bits"


# ---------------------------------------------------------------------------
# the cases

def _zero_negative_diagonal():
    # row 0: (-2 + 1) + 1 == 0 -> d_0 = 0; node 0 is also a column of row 3
    return from_entries(6, {(0, 0): -2.0, (0, 3): 1.0, (3, 0): 1.0, (1, 2): 2.0, (2, 1): 2.0,
                            (4, 5): 1.0, (5, 4): 1.0})


def _zero_by_cancellation():
    # row 2: 1 - 2 + [1] == 0 among off-diagonals; rows 0, 1, 4 use node 2
    return from_entries(5, {(2, 0): 1.0, (2, 1): -2.0, (0, 2): 1.0, (1, 2): 2.0,
                            (4, 2): 3.0, (3, 4): 1.0, (4, 3): 1.0})


def _zero_rows_first_last():
    # rows 0, 3, 4 and 7 (first and last) sum to 0; every one of them is a
    # column of a row that does not
    e = {(0, 0): -3.0, (0, 1): 1.0, (0, 5): 1.0,            # -2 + 1 + 1
         (3, 1): -1.0,                                       # -1 + [1]
         (4, 4): -1.5, (4, 5): 0.25, (4, 6): 0.25,           # -.5 + .25 + .25
         (7, 2): 2.0, (7, 6): -3.0,                          # 2 - 3 + [1]
         (1, 0): 1.0, (1, 3): 1.0, (2, 4): 1.0, (2, 7): 1.0, (5, 0): 2.0, (5, 7): 1.0,
         (6, 3): 1.0, (6, 4): 1.0, (6, 5): 1.0}
    return from_entries(8, e)


def _lone_negative_diagonal():
    # row 2 of A+I is empty (its only entry -1 + 1 is pruned): sum 0, d = 0
    return from_entries(4, {(2, 2): -1.0, (0, 2): 1.0, (1, 2): 1.0, (1, 3): 1.0, (3, 1): 1.0})


def _negative_identity():
    return from_entries(5, {(i, i): -1.0 for i in range(5)})


def _all_rows_zero():
    # a ring of -1: every row is [1] - 1 == 0, so every d is 0 and S is empty
    return from_entries(4, {(i, (i + 1) % 4): -1.0 for i in range(4)})


def _signed_integers(n=200, per_row=10, seed=20):
    """Integer weights in [-2, 2] (stored zeros included): negative row sums
    give NaN d, zero row sums give d = 0."""
    rng = np.random.default_rng(seed)
    e = {}
    for i in range(n):
        for j in rng.choice(n, per_row, replace=False):
            e[(i, int(j))] = float(rng.integers(-2, 3))
    return from_entries(n, e)


def _special_weights():
    """+-inf, NaN and 1e+-200 weights; rows whose sum is +inf, -inf (d = 0),
    NaN (inf - inf, a NaN weight, a negative sum) or finite, each also a
    column of rows of every other kind."""
    n = 10
    e = {(0, 1): INF, (0, 5): 1.0, (0, 9): 2.0,                    # sum +inf
         (1, 0): -INF, (1, 6): 1.0,                                # sum -inf
         (2, 0): INF, (2, 1): -INF, (2, 7): 1.0,                   # sum NaN (inf - inf)
         (3, 4): NAN, (3, 5): 1.0, (3, 0): 2.0,                    # sum NaN (NaN weight)
         (4, 4): INF, (4, 0): 1.0, (4, 3): 1.0,                    # inf on the diagonal
         (5, 0): 1.0, (5, 1): 1.0, (5, 2): 1.0, (5, 3): 1.0, (5, 6): 1e200,   # finite, huge
         (6, 0): 1e-200, (6, 2): 1e-200, (6, 5): 1e-200, (6, 4): 1.0,         # finite
         (7, 7): -5.0, (7, 0): 1.0, (7, 2): 1.0, (7, 5): 1.0, (7, 6): 1.0,    # negative: NaN d
         (8, 7): 1.0, (8, 3): 1.0, (8, 4): 1.0, (8, 1): 1.0, (8, 9): 1e-200,
         (9, 9): NAN, (9, 0): 1.0, (9, 8): 1.0}                    # NaN on the diagonal
    return from_entries(n, e)


def _rounding():
    """Products that are nonzero in fp64 and 0.0f, subnormal or +-inf in fp32,
    each in a row that also has a true zero product (column 0 has d = 0) and
    in a row that has none; products that underflow fp64 itself at the first
    or at the second multiplication; and a row with a large d_i where
    d_i * (a * d_j) underflows and (d_i * a) * d_j does not."""
    e = {(0, 0): -1.0,                                             # d_0 = 0
         (1, 9): 1e300,                                            # d_1 = 1e-150
         (2, 9): 1e200,                                            # d_2 = 1e-100
         # with a true zero product (column 0)
         (3, 0): 1.0, (3, 4): 1e-60, (3, 5): 1e-40, (3, 6): -1e-41,
         (4, 0): 1.0, (4, 9): 1e300, (4, 8): -0.5e300,             # +-inf in fp32, d_9 = d_8 = 1
         # without one
         (5, 4): 1e-60, (5, 6): 1e-40, (5, 7): -1e-41, (5, 3): -1e-60,
         (6, 9): 1e300, (6, 8): -0.5e300,
         # fp64 underflow: 1e-100 * 1e-300 == 0 (first product), and
         # (d_7 * 1e-200) * 1e-150 == 0 (second product); neither row is flagged otherwise
         (2, 3): 1e-300,
         (7, 1): 1e-200, (7, 2): 1e-60,
         # d_10 = 2^26: (d * 1e-180) * 1e-150 is a nonzero subnormal, d * (1e-180 * 1e-150) is 0
         (10, 10): -1.0 + 2.0 ** -52, (10, 1): 1e-180, (10, 5): 1e-190}
    return from_entries(11, e)


def _stored_zeros():
    """Stored 0.0 and -0.0 on and off the diagonal: A+I prunes them off the
    diagonal (a + 0 == 0) and turns them into 1.0 on it.  Row 4 has a negative
    sum (NaN d): a zero kept there would survive as NaN * 0."""
    e = {(0, 0): 0.0, (0, 2): -0.0, (0, 3): 1.0,
         (1, 1): -0.0, (1, 0): 0.0, (1, 4): 1.0,
         (2, 0): 0.0, (2, 1): -0.0,
         (3, 0): 1.0, (3, 5): 0.0,
         (4, 4): -3.0, (4, 1): 0.0, (4, 2): 1.0, (4, 5): -0.0,
         (5, 4): 1.0, (5, 5): 0.0}
    return from_entries(6, e)


def _zero_diag_row():
    # the graph of tests/test_gpu_normalize.py's case of this name
    return from_entries(6, {(0, 0): -1.0, (0, 3): 1.0, (1, 2): 2.0, (2, 1): 2.0})


def _pruned_diagonal():
    # a_ii + 1 == 0 as the first, a middle and the last entry of its row
    return from_entries(5, {(0, 0): -1.0, (0, 2): 1.0, (0, 4): 2.0,
                            (2, 0): 1.0, (2, 2): -1.0, (2, 3): 2.0,
                            (4, 1): 1.0, (4, 3): 2.0, (4, 4): -1.0,
                            (1, 0): 1.0, (3, 4): 1.0})


def _absent_diagonal():
    # no stored diagonal: columns all below i, all above i, both; rows 0 and n-1
    return from_entries(6, {(0, 2): 1.0, (0, 5): 2.0,              # row 0, all above
                            (1, 3): 1.0, (1, 4): 1.0,              # all above
                            (3, 0): 1.0, (3, 1): 3.0,              # all below
                            (4, 0): 1.0, (4, 5): 1.0,              # both sides
                            (5, 0): 2.0, (5, 3): 1.0})             # row n-1, all below
    # row 2 has no entry at all


def _sum_order():
    """Row sums that depend on the order, the precision and the place of the
    diagonal.  Rows 0..3 are plain (d = 1 or so); the rows below are built as
    [BIG, ones..., -BIG, 3, 3]: left to right the ones are absorbed by BIG.

    row 10  diagonal absent, its sorted place between BIG and -BIG (absorbed)
    row 11  the same entries with the diagonal stored (as 0.0)
    row 12  BIG32 in place of BIG: exact in fp64, absorbed in fp32
    row 300 250 entries: numpy's pairwise sum keeps the ones in other lanes
    """
    n = 301
    e = {(0, 1): 1.0, (1, 0): 1.0, (2, 3): 1.0, (3, 2): 1.0}
    e.update({(10, 2): BIG, (10, 5): 1.0, (10, 7): 1.0, (10, 12): 1.0, (10, 20): -BIG,
              (10, 21): 3.0, (10, 22): 3.0})
    e.update({(11, 2): BIG, (11, 5): 1.0, (11, 11): 0.0, (11, 12): 1.0, (11, 20): -BIG,
              (11, 21): 3.0, (11, 22): 3.0})
    e.update({(12, 2): BIG32, (12, 5): 1.0, (12, 7): 1.0, (12, 13): 1.0, (12, 20): -BIG32,
              (12, 21): 3.0})
    e[(300, 0)] = BIG
    for j in range(1, 247):
        e[(300, j)] = 1.0
    e[(300, 247)] = -BIG
    e[(300, 248)] = 3.0
    e[(300, 249)] = 3.0
    A = from_entries(n, e)
    for i in (10, 11, 300):
        _, v = aplus_i_row(A, i)
        s = sequential_sum(v)
        assert s != sequential_sum(v[::-1]), i
        assert s > 0 and sequential_sum(v[::-1]) > 0, i
    _, v = aplus_i_row(A, 10)
    _, v_last = aplus_i_row(A, 10, diagonal="last")
    assert sequential_sum(v) != sequential_sum(v_last)
    _, v = aplus_i_row(A, 12)
    assert sequential_sum(v) != sequential_sum(v, np.float32) and sequential_sum(v, np.float32) > 0
    _, v = aplus_i_row(A, 300)
    assert len(v) >= 200 and sequential_sum(v) != np.sum(v) and np.sum(v) > 0
    return A


_BUILDERS = {
    "zero_negative_diagonal": _zero_negative_diagonal,
    "zero_by_cancellation": _zero_by_cancellation,
    "zero_rows_first_last": _zero_rows_first_last,
    "lone_negative_diagonal": _lone_negative_diagonal,
    "negative_identity": _negative_identity,
    "all_rows_zero": _all_rows_zero,
    "signed_integers": _signed_integers,
    "special_weights": _special_weights,
    "rounding": _rounding,
    "stored_zeros": _stored_zeros,
    "zero_diag_row": _zero_diag_row,
    "pruned_diagonal": _pruned_diagonal,
    "absent_diagonal": _absent_diagonal,
    "sum_order": _sum_order,
}
CASE_NAMES = tuple(_BUILDERS)
SUBGRAPH_CASE = "signed_integers"
PROPAGATION_CASES = ("signed_integers", "zero_rows_first_last", "rounding")


def row_sums(A):
    return np.array([sequential_sum(aplus_i_row(A, i)[1]) for i in range(A.shape[0])])


@functools.lru_cache(maxsize=None)
def _cases():
    out = {name: build() for name, build in _BUILDERS.items()}
    # what the cases are for, checked here and not left to luck
    s = row_sums(out["signed_integers"])
    A = out["signed_integers"]
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    zero, neg = s == 0, s < 0
    assert (zero[rows] & neg[A.indices] & (A.data != 0)).any()    # d_i = 0, d_j = NaN
    assert (neg[rows] & zero[A.indices] & (A.data != 0)).any()    # d_i = NaN, d_j = 0
    assert (A.data == 0).any()
    s = row_sums(out["special_weights"])
    assert np.isposinf(s).any() and np.isneginf(s).any() and np.isnan(s).any() \
        and (s < 0).any() and (np.isfinite(s) & (s > 0)).any()
    for name in ("zero_negative_diagonal", "zero_by_cancellation", "zero_rows_first_last",
                 "lone_negative_diagonal", "rounding"):
        s = row_sums(out[name])
        assert (s == 0).any() and (s != 0).any(), name
        assert np.isin(out[name].indices, np.nonzero(s == 0)[0]).any(), name
    s = row_sums(out["zero_rows_first_last"])
    assert s[0] == 0 and s[-1] == 0 and (s == 0).sum() >= 3
    assert not row_sums(out["negative_identity"]).any() and not row_sums(out["all_rows_zero"]).any()
    assert row_sums(out["zero_diag_row"])[0] == 1.0    # a_00 + 1 is pruned, a_03 = 1 stays
    return out


def cases():
    """{name: scipy CSR}; fresh copies, so a test may change what it gets."""
    return {k: v.copy() for k, v in _cases().items()}


def subgraph_index(n, seed=3):
    """A shuffled 60% of the nodes: the train index of the slice-then-normalise case."""
    return np.random.default_rng(seed).permutation(n)[:int(0.6 * n)].astype(np.int64)


# ---------------------------------------------------------------------------
# the sub-graph kernels' source graph

SUB_ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)
SUB_PATTERN_COLS = 1024        # columns 0..1023 carry the keep patterns, 64 per chunk
SUB_N = SUB_PATTERN_COLS + 112
SUB_FIRST_ROW = SUB_PATTERN_COLS   # rows of the exact lengths, then 100 richer rows
SUB_SPECIALS = np.array([0.0, -0.0, NAN, INF, -INF, 1e-300, -1e300])


def _kept_pattern():
    """keep[c] for pattern columns: chunk 0 none, 1 all, 2 alternating, 3 only
    lane 0, 4 only lane 63, 5-6 a run that crosses the chunk edge, then
    seeded random chunks."""
    keep = np.zeros(SUB_PATTERN_COLS, bool)
    keep[64:128] = True
    keep[128:192:2] = True
    keep[192] = True
    keep[256 + 63] = True
    keep[320 + 40:384 + 20] = True
    rng = np.random.default_rng(8)
    keep[448:] = rng.random(SUB_PATTERN_COLS - 448) < 0.4
    return keep


@functools.lru_cache(maxsize=None)
def _subgraph_source():
    rng = np.random.default_rng(9)
    n = SUB_N
    indptr, indices = [0], []
    for i in range(n):
        if i < SUB_PATTERN_COLS:           # a few entries each, both halves
            cols = np.unique(np.concatenate([rng.integers(0, n, 3),
                                             rng.integers(SUB_FIRST_ROW, n, 2)]))
        elif i - SUB_FIRST_ROW < len(SUB_ROW_LENGTHS):
            length = SUB_ROW_LENGTHS[i - SUB_FIRST_ROW]
            start = {63: 64, 65: 32, 129: 100}.get(length, 0)   # aligned and unaligned to the pattern
            cols = np.arange(start, start + length)
        else:                               # rows that stay non-empty under a small idx
            cols = np.unique(np.concatenate([rng.integers(SUB_FIRST_ROW, n, 40),
                                             rng.integers(0, SUB_PATTERN_COLS, 30)]))
        indices.append(cols)
        indptr.append(indptr[-1] + len(cols))
    indices = np.concatenate(indices)
    data = rng.standard_normal(len(indices))
    special = rng.random(len(indices)) < 0.08
    data[special] = rng.choice(SUB_SPECIALS, int(special.sum()))
    A = from_arrays(n, np.array(indptr), indices, data)
    lengths = np.diff(A.indptr)[SUB_FIRST_ROW:SUB_FIRST_ROW + len(SUB_ROW_LENGTHS)]
    assert tuple(lengths) == SUB_ROW_LENGTHS
    kept = np.concatenate([np.nonzero(_kept_pattern())[0], np.arange(SUB_FIRST_ROW, n)])
    return A, kept.astype(np.int64)


def subgraph_source():
    """(A, kept): the graph and the ascending node set whose membership gives
    the long rows their per-chunk keep patterns."""
    A, kept = _subgraph_source()
    return A.copy(), kept.copy()


def subgraph_small_index(m, seed=1):
    """m shuffled ids among the richer rows (entries survive a small idx);
    m of 2^k - 1, 2^k, 2^k + 1 sits on the edge of the sort's key bits."""
    first = SUB_FIRST_ROW + len(SUB_ROW_LENGTHS)
    ids = np.random.default_rng(seed).permutation(np.arange(first, SUB_N))[:m]
    assert len(ids) == m
    if m > 1 and np.all(np.diff(ids) > 0):
        ids = ids[::-1].copy()
    return ids.astype(np.int64)
