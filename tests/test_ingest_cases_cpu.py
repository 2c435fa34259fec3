"""The ingest and sort boundary cases (ingest_cases.py) without a GPU.

* a numpy model of csrc/sort.hip as written equals the stable numpy sort on
  every case, the two past the scan's carry step included;
* one-line mutants of that model each differ from the reference on the
  cases ingest_cases.KILLED_BY names -- which is what shows that the same
  cases, run on the device (test_gpu_ingest.py), would catch the same fault
  in the kernels.  The mutants run on every case below 20,000 pairs and on
  the larger ones the table names for them (a model run of 4.2 million pairs
  takes about two seconds);
* sgc_coo_to_csr_cpu and the test oracle's coo_to_csr are held to the same
  reference: arrays, value bits and status.
"""
import ctypes

import numpy as np
import pytest

import ingest_cases as ic

BIG_MODEL = 20000


@pytest.fixture(scope="module", autouse=True)
def _lib_built():
    from sgc_amd import build
    build.build(verbose=False)


@pytest.fixture(scope="module")
def refs():
    """{case: (Coo, Ref)}: every reference is computed once and only read."""
    out = {}
    for name in ic.COO_CASES:
        case = ic.coo_case(name)
        ref = ic.reference(*case)
        for a in (*case[:3], *ref[:3]):
            a.setflags(write=False)
        out[name] = (case, ref)
    return out


def same_csr(got, ref):
    rp, ci, va = got
    return (rp is not None and np.array_equal(rp, ref.row_ptr) and np.array_equal(ci, ref.col)
            and ci.dtype == np.int32 and np.array_equal(ic.bits(va), ic.bits(ref.val)))


def coo_differs(case, ref, mutant):
    try:
        return not same_csr(ic.model_coo_to_csr(case, mutant), ref)
    except ic.ModelFault:
        return True


def plan_differs(deg, mutant):
    try:
        return not np.array_equal(ic.model_plan_sorted(deg, mutant),
                                  np.argsort(-deg, kind="stable"))
    except ic.ModelFault:
        return True


# ---------------------------------------------------------------------------
# the cases are what their names say

def test_cases_reach_the_boundaries_they_name(refs):
    for name, want in ic.EXPECTED_STATUS.items():
        assert refs[name][1].status == want, name
    for name, (case, ref) in refs.items():
        assert case.vals.dtype == np.float32 and len(np.unique(ic.bits(case.vals))) == len(case.vals)
        unsorted = not ref.status & ic.ROWS_SORTED
        assert unsorted == (not name.startswith(("sorted_gaps", "nnz_edges[1]", "wrap_violation[wrap_e"))
                            and name != "one_key_many_tiles"), name
    assert len(refs["scan_carry"][0].rows) > 2048 * 2048             # more than 1,024 scan blocks
    hub = np.bincount(refs["scan_carry"][0].rows).max()
    assert hub >= len(refs["scan_carry"][0].rows) // 8
    for n in ic.PASS_BOUNDARY_ROWS:
        rows = refs[f"pass_boundaries[{n}]"][0].rows
        assert set(ic.pass_boundary_required_rows(n)) <= set(rows.tolist())
        assert {0, 2047, n - 1} <= set(ic.pass_boundary_required_rows(n))
    k = ic.GRID_THREADS - 1
    for name, at in (("wrap_violation[wrap]", k), ("wrap_violation[block]", 255)):
        rows = refs[name][0].rows
        assert np.flatnonzero(np.diff(rows) < 0).tolist() == [at], name   # the one violation
    case = refs["wrap_violation[wrap_equal_columns]"][0]
    same = (np.diff(case.rows) == 0) & (np.diff(case.cols) <= 0)
    assert np.flatnonzero(same).tolist() == [k]
    gaps = np.diff(refs["sorted_gaps[10000]"][1].row_ptr)
    assert not gaps[:100].any() and not gaps[-100:].any() and not gaps[2400:7400].any()
    assert gaps[100] or gaps[101] or gaps[102]
    special = ic.bits(refs["special_value_bits"][0].vals)
    assert {0x7f800000, 0xff800000, 0x80000000, 0x7f800001, 0xffc00000} <= set(special.tolist())
    for deg in (ic.plan_scan_carry(), ic.plan_scan_carry(True)):
        assert len(deg) == 2048 * 2048 + 3 and (deg == 3000).sum() == 3 and deg.sum() < 2 ** 31
    assert len(ic.narrowing()) == 12 and len(ic.bad_crow()) == 7
    for name, case in ic.narrowing().items():
        assert ic.reference(*case).status & ic.OUT_OF_RANGE, name
        r32, c32 = case.rows.astype(np.int32), case.cols.astype(np.int32)   # ... and fit once cut
        if "2^31" not in name:
            assert ((r32 >= 0) & (r32 < 8) & (c32 >= 0) & (c32 < 8)).all(), name


# ---------------------------------------------------------------------------
# the model of sort.hip

@pytest.mark.parametrize("name", list(ic.COO_CASES))
def test_sort_model_equals_reference(refs, name):
    case, ref = refs[name]
    assert same_csr(ic.model_coo_to_csr(case), ref)


@pytest.mark.parametrize("name", list(ic.PLAN_CASES))
def test_sort_model_descending_equals_reference(name):
    deg = ic.PLAN_CASES[name]()
    assert np.array_equal(ic.model_plan_sorted(deg), np.argsort(-deg, kind="stable"))


@pytest.mark.parametrize("name", list(ic.SMALL_CASES) + ["plan_small"])
def test_stepwise_model_equals_vectorised_model(refs, name):
    """The model's two forms of a pass -- every pair at once, and tile by
    tile with next-slot counters as the kernel steps -- agree, so the mutant
    that needs the second form (f) is a mutant of the same model."""
    if name in ic.PLAN_CASES:
        deg = ic.PLAN_CASES[name]()
        assert np.array_equal(ic.model_plan_sorted(deg, stepwise=True), ic.model_plan_sorted(deg))
    else:
        case, ref = refs[name]
        assert same_csr(ic.model_coo_to_csr(case, stepwise=True), ref)


@pytest.fixture(scope="module")
def caught(refs):
    """{mutant: [cases whose result it changes]}, computed once."""
    out = {m: [] for m in ic.MUTANTS}
    for m in ic.MUTANTS:
        named = ic.KILLED_BY.get(m, ())
        for name, (case, ref) in refs.items():
            if (len(case.rows) < BIG_MODEL or name in named) and coo_differs(case, ref, m):
                out[m].append(name)
        for name, build in ic.PLAN_CASES.items():
            if (name not in ic.BIG_PLAN_CASES or name in named) and plan_differs(build(), m):
                out[m].append(name)
    return out


@pytest.mark.parametrize("mutant", [m for m in ic.MUTANTS if m not in ic.EQUIVALENT_MUTANTS])
def test_mutant_of_the_sort_is_caught(caught, mutant):
    print(f"mutant ({mutant}) {ic.MUTANTS[mutant]}: caught by {', '.join(caught[mutant]) or 'NOTHING'}")
    assert caught[mutant], f"no case catches mutant ({mutant}): {ic.MUTANTS[mutant]}"
    for name in ic.KILLED_BY[mutant]:
        assert name in caught[mutant], f"{name} does not catch mutant ({mutant})"


def test_carry_mutant_needs_the_last_bin(caught):
    """The carried step of the block-sum scan is only visible where a digit of
    the last scan block is in use: plan_scan_carry as first specified computes
    the carry and never reads it, its last_bin variant does."""
    assert "plan_scan_carry[last_bin]" in caught["c"]
    assert not plan_differs(ic.plan_scan_carry(), "c")
    assert set(caught["c"]) == set(ic.KILLED_BY["c"])


def test_complement_mutant_is_no_fault(caught):
    """(g) `~key` for `key_max - key`: proved equivalent in ingest_cases.py
    (every key is below 2^(11 * passes)), so no case is asked to catch it;
    what is checked is that it really changes nothing at one, two and three
    passes and at key_max either side of a digit -- if it ever does, the
    proof's premise broke and the mutant belongs in KILLED_BY."""
    assert caught["g"] == []
    rng = np.random.default_rng(19)
    for top in (0, 1, 2047, 2048, 2 ** 22 - 1, 2 ** 22, 5_000_000, 2 ** 31 - 2):
        deg = rng.integers(0, top + 1, 3000)
        deg[[5, 1700, 2999]] = top
        deg[[6, 1701]] = 0
        assert not plan_differs(deg, "g"), top
        assert top == 0 or plan_differs(deg, "h"), top


# ---------------------------------------------------------------------------
# the host ingest and the oracle against the same reference

def _cpu_ingest(case, with_status=True):
    from sgc_amd import _lib
    lib = _lib.load()
    rows, cols = np.ascontiguousarray(case.rows), np.ascontiguousarray(case.cols)
    vals = np.ascontiguousarray(case.vals)
    nnz, pad = len(rows), 3
    row_ptr = np.full(case.n_rows + 1 + pad, -7, np.int32)
    col = np.full(nnz + pad, -7, np.int32)
    val = np.full(nnz + pad, 0x7fc0dead, np.uint32)
    status = ctypes.c_uint32(0xffffffff)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.sgc_coo_to_csr_cpu(p(rows), p(cols), p(vals), nnz, case.n_rows, case.n_cols,
                                p(row_ptr), p(col), p(val),
                                ctypes.byref(status) if with_status else None)
    if rc == 0:     # nothing past the arrays
        assert (row_ptr[case.n_rows + 1:] == -7).all() and (col[nnz:] == -7).all()
        assert (val[nnz:] == 0x7fc0dead).all()
    return rc, status.value, (row_ptr[:case.n_rows + 1], col[:nnz], val[:nnz].view(np.float32))


@pytest.mark.parametrize("name", list(ic.COO_CASES))
def test_host_ingest_equals_reference(refs, name):
    case, ref = refs[name]
    rc, status, got = _cpu_ingest(case)
    assert rc == 0 and same_csr(got, ref)
    assert status == ref.status, f"status {status}, the reference has {ref.status}"


@pytest.mark.parametrize("name", list(ic.narrowing()))
def test_host_ingest_refuses_indices_that_only_fit_once_narrowed(name):
    from sgc_amd import _lib
    SGC_ERANGE = 2
    rc, status, _ = _cpu_ingest(ic.narrowing()[name])
    assert rc == SGC_ERANGE and status & ic.OUT_OF_RANGE
    assert _lib.load().sgc_last_error()
    assert _cpu_ingest(ic.narrowing()[name], with_status=False)[0] == SGC_ERANGE


@pytest.mark.parametrize("name", ["one_key_many_tiles", "one_key_many_tiles[after_a_later_row]",
                                  "column_major[400x300]", "column_major[300x400]", "reverse_rows",
                                  "special_value_bits"])
def test_oracle_ingest_equals_reference(refs, oracle, name):
    """Half the device tests take oracle.coo_to_csr as their expected CSR;
    this ties it to the numpy rule."""
    case, ref = refs[name]
    assert same_csr(oracle.coo_to_csr(case.n_rows, case.n_cols, case.rows, case.cols, case.vals), ref)
