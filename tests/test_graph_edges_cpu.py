"""Graph construction on the host against the reference's own S.

tests/golden/graph_edges.npz holds, for every case of graph_edge_cases.py,
what the reference's aug_normalized_adjacency + sparse_mx_to_torch_sparse_tensor
returned.  Checked against it here, without a GPU:

* sgc_amd.normalization.aug_normalized_adjacency (the --no-cuda loader path
  and the checker of the randomised device tests);
* a numpy model of the device recipe (csrc/normalize.hip): one row at a time,
  diagonal inserted at its sorted position, sequential fp64 sum, d from
  _inv_power, the four-part drop rule, one rounding to fp32;
* mutants of that model, each of which must differ from the reference on a
  named case -- which is what shows the cases would catch the same error in
  the kernels.
"""
import os

import numpy as np
import pytest

import graph_edge_cases as g

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_edges.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_case(golden, name):
    n = len(golden[f"{name}/indptr"]) - 1
    A = g.from_arrays(n, golden[f"{name}/indptr"], golden[f"{name}/indices"], golden[f"{name}/data"])
    return A, tuple(golden[f"{name}/{k}"] for k in ("row", "col", "val"))


def f32(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float32)


def test_fixture_holds_the_builder_cases(golden):
    """The stored inputs are the builder's (bit for bit), so the fixture's
    outputs belong to the cases the module documents."""
    built = g.cases()
    assert {k.split("/")[0] for k in golden} == set(g.CASE_NAMES) | {"sub"}
    for name, A in built.items():
        assert np.array_equal(golden[f"{name}/indptr"], A.indptr), name
        assert np.array_equal(golden[f"{name}/indices"], A.indices), name
        assert np.array_equal(golden[f"{name}/data"].view(np.uint64), A.data.view(np.uint64)), name
    assert np.array_equal(golden["sub/idx"], g.subgraph_index(built[g.SUBGRAPH_CASE].shape[0]))
    assert len(golden["negative_identity/row"]) == 0 and len(golden["all_rows_zero/row"]) == 0


def test_rounding_case_reaches_every_fp32_edge(golden):
    """The reference's S of the rounding case keeps 0.0f, subnormal and +-inf
    entries both in rows that also lose an entry to a d = 0 column (3, 4) and
    in rows that lose none (5, 6), and loses the two fp64 underflows."""
    row, col, val = (golden[f"rounding/{k}"] for k in ("row", "col", "val"))
    tiny = np.float32(2.0 ** -126)
    for rows in ((3, 4), (5, 6)):
        v = val[np.isin(row, rows)]
        assert (v == 0).any() and ((v != 0) & (np.abs(v) < tiny)).any(), rows
        assert np.isposinf(v).any() and np.isneginf(v).any(), rows
    have = set(zip(row.tolist(), col.tolist()))
    assert (3, 0) not in have and (4, 0) not in have          # true zero products
    assert (2, 3) not in have and (7, 1) not in have          # d_i * a == 0, (d_i * a) * d_j == 0
    assert (10, 1) in have and val[(row == 10) & (col == 1)][0] == 0   # kept: (d * a) * d_j != 0


@pytest.mark.parametrize("name", g.CASE_NAMES)
def test_host_augnorm_matches_reference(golden, name):
    from sgc_amd.normalization import aug_normalized_adjacency
    A, want = golden_case(golden, name)
    got = aug_normalized_adjacency(A)
    assert got.getformat() == "coo" and got.shape == A.shape
    g.compare_s(got.row, got.col, f32(got.data), *want, what=name)


def test_host_subgraph_then_augnorm_matches_reference(golden):
    from sgc_amd.normalization import aug_normalized_adjacency
    A, _ = golden_case(golden, g.SUBGRAPH_CASE)
    idx = golden["sub/idx"]
    got = aug_normalized_adjacency(A[idx, :][:, idx])
    g.compare_s(got.row, got.col, f32(got.data),
                golden["sub/row"], golden["sub/col"], golden["sub/val"], what="sub")


# ---------------------------------------------------------------------------
# the device recipe as a numpy model, and its mutants

def device_model(A, prune="four_part", diagonal="sorted", order="sequential",
                 sum_dtype=np.float64, association="left", stored_zeros=False):
    from sgc_amd.normalization import _inv_power
    n = A.shape[0]
    rows_of = [g.aplus_i_row(A, i, diagonal=diagonal, stored_zeros=stored_zeros) for i in range(n)]
    rowsum = np.zeros(n, np.float64)
    for i, (_, v) in enumerate(rows_of):
        if order == "sequential":
            rowsum[i] = g.sequential_sum(v, sum_dtype)
        elif order == "reversed":
            rowsum[i] = g.sequential_sum(v[::-1], sum_dtype)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                rowsum[i] = np.sum(v) if len(v) else 0.0
    with np.errstate(invalid="ignore"):
        d = _inv_power(rowsum.copy(), -0.5)
    out_r, out_c, out_v = [], [], []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, (cols, vals) in enumerate(rows_of):
            if diagonal == "last":      # the diagonal's place in S stays sorted
                o = np.argsort(cols, kind="stable")
                cols, vals = cols[o], vals[o]
            di, dj = d[i], d[cols]
            if association == "left":
                t = di * vals
                s = t * dj
            else:
                t = vals * dj
                s = di * t
            s32 = s.astype(np.float32)
            if prune == "four_part":
                keep = (di != 0.0) & (dj != 0.0) & (t != 0.0) & (s != 0.0)
            elif prune == "final_product":
                keep = s != 0.0
            elif prune == "rounded_in_flagged_rows":
                keep = (s32 != 0.0) | ~np.any(s == 0.0)
            else:
                keep = np.ones(len(s), bool)
            out_r.append(np.full(int(keep.sum()), i, np.int64))
            out_c.append(cols[keep])
            out_v.append(s32[keep])
    cat = (lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt))
    return cat(out_r, np.int64), cat(out_c, np.int64), cat(out_v, np.float32)


@pytest.mark.parametrize("name", g.CASE_NAMES)
def test_device_recipe_model_matches_reference(golden, name):
    A, want = golden_case(golden, name)
    g.compare_s(*device_model(A), *want, what=name)


MUTANTS = {
    # the first three are what the code did before the drop rule was restated
    "prune on the final product only": dict(prune="final_product"),
    "prune on the fp32 value in flagged rows": dict(prune="rounded_in_flagged_rows"),
    "no pruning": dict(prune="none"),
    "diagonal appended last": dict(diagonal="last"),
    "reversed sum order": dict(order="reversed"),
    "pairwise np.sum": dict(order="pairwise"),
    "fp32 row sum": dict(sum_dtype=np.float32),
    "d_i * (a * d_j)": dict(association="right"),
    "stored zeros counted": dict(stored_zeros=True),
}
# the cases that must catch the three former behaviours, named by the kind of graph
MUST_CATCH = {
    "prune on the final product only": ("signed_integers", "special_weights"),
    "prune on the fp32 value in flagged rows": ("rounding",),
    "no pruning": ("zero_negative_diagonal", "zero_by_cancellation", "zero_rows_first_last",
                   "lone_negative_diagonal", "all_rows_zero"),
}


def _differs(golden, name, **mutant):
    A, want = golden_case(golden, name)
    try:
        g.compare_s(*device_model(A, **mutant), *want, what=name)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_of_the_recipe_is_caught(golden, mutant):
    caught = [name for name in g.CASE_NAMES if _differs(golden, name, **MUTANTS[mutant])]
    print(f"mutant '{mutant}' caught by: {', '.join(caught) or 'NOTHING'}")
    assert caught, f"no case catches the mutant '{mutant}'"
    for name in MUST_CATCH.get(mutant, ()):
        assert name in caught, f"case {name} does not catch the mutant '{mutant}'"
