"""Inputs that take the ingest and the library's radix sort through their
boundaries.

Every call into the library starts with sgc_coo_to_csr / sgc_csr64_to_csr
(csrc/ingest.hip) and the stable LSD radix sort of csrc/sort.hip, which
sgc_plan_sorted uses too.  A wrong permutation there corrupts every later
result without an error.  The sizes at which that code changes path:

  64 / 512 / 2,048     pairs per ballot chunk / wave portion / tile of the sort
  11 bits              per digit: one pass up to key_max 2,047, two up to
                       2^22 - 1, three above (key_max = n_rows - 1 in the ingest,
                       the longest row in the plan)
  4,096 / 1,024        counts per scan block / block sums per step of the
                       carried scan: more than 1,024 scan blocks = more than
                       2,048 tiles = more than 2,048 x 2,048 pairs
  8,192 x 256          threads of the ingest's largest grid (grid-stride wrap)

reference              the rule: a stable numpy sort by row, the three status bits
COO_CASES / coo_case   {name: builder} of COO inputs, deterministic, inputs only
plan_scan_carry        degrees for sgc_plan_sorted past the scan's carry step
bad_crow / narrowing   inputs every ingest must refuse
radix_sort_model       csrc/sort.hip as written, in numpy, and its MUTANTS;
                       KILLED_BY records which case catches which mutant

Plain numpy; no GPU, no native library, no pytest.
"""
import functools
from collections import namedtuple

import numpy as np

ROWS_SORTED, COLS_ASCENDING, OUT_OF_RANGE = 1, 2, 4

Coo = namedtuple("Coo", "rows cols vals n_rows n_cols")
Ref = namedtuple("Ref", "row_ptr col val status")


def order_bits(nnz):
    """fp32 values whose bit patterns are 0, 1, 2, ...: all distinct (denormals
    from 1 on), so a misplaced or altered entry cannot hide."""
    return np.arange(nnz, dtype=np.int32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def reference(rows, cols, vals, n_rows, n_cols):
    """The CSR of a COO: every entry kept, stable by row; and the status word:
    bit 1 iff rows is non-decreasing, bit 2 iff every CSR row is strictly
    ascending, bit 4 iff any index is out of range (no arrays then)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32)
    status = ROWS_SORTED if bool(np.all(np.diff(rows) >= 0)) else 0
    if ((rows < 0) | (rows >= n_rows) | (cols < 0) | (cols >= n_cols)).any():
        return Ref(None, None, None, status | OUT_OF_RANGE)
    order = np.argsort(rows, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int32)
    col = cols[order]
    same_row = np.diff(rows[order]) == 0
    if bool(np.all(np.diff(col)[same_row] > 0)):
        status |= COLS_ASCENDING
    return Ref(row_ptr, col.astype(np.int32), vals[order], status)


def reference_csr(crow, col, vals, n_cols):
    """What sgc_csr64_to_csr owes for a valid CSR: the arrays narrowed, bit 1
    always, bit 2 iff every row is strictly ascending."""
    crow, col = np.asarray(crow, np.int64), np.asarray(col, np.int64)
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    ref = reference(rows, col, vals, len(crow) - 1, n_cols)
    assert ref.status & ROWS_SORTED and np.array_equal(ref.row_ptr, crow)
    return ref


# ---------------------------------------------------------------------------
# COO cases

NNZ_EDGES = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)
PASS_BOUNDARY_ROWS = (2048, 2049, 2 ** 22, 2 ** 22 + 1)
GRID_THREADS = 8192 * 256            # check_narrow_kernel's largest grid
WRAP_NNZ = GRID_THREADS + 300
SCAN_CARRY_NNZ = 2048 * 2048 + 1 + 2048


def _coo(rows, cols, n_rows, n_cols, vals=None):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    return Coo(rows, cols, order_bits(len(rows)) if vals is None else vals, n_rows, n_cols)


def nnz_edges(nnz):
    """Unsorted rows over 300 rows, nnz either side of a chunk, a wave
    portion, a tile and two tiles."""
    rng = np.random.default_rng(1000 + nnz)
    rows = rng.integers(0, 300, nnz)
    if nnz > 1:
        rows[0], rows[-1] = 299, 0
    return _coo(rows, rng.integers(0, 200, nnz), 300, 200)


def one_key_many_tiles(lead=False):
    """Every entry in row 5 of 9 rows, three whole tiles and a piece: the
    order inside the key rests on the wave bases and the tiles' offsets.
    lead: one entry of row 8 first, so that the rows are unsorted and the
    device ingest sorts (tiles 1 and 2 are still one key)."""
    rng = np.random.default_rng(11)
    nnz = 3 * 2048 + 17
    rows = np.full(nnz, 5)
    if lead:
        rows = np.concatenate([[8], rows])
    return _coo(rows, rng.integers(0, 40, len(rows)), 9, 40)


def two_keys_interleaved():
    nnz = 2 * 2048 + 1
    rng = np.random.default_rng(12)
    return _coo(1 - np.arange(nnz) % 2, rng.integers(0, 64, nnz), 2, 64)


def reverse_rows():
    """Rows 4999 .. 0, twice: two passes, every key twice, a tile apart."""
    rng = np.random.default_rng(13)
    rows = np.tile(np.arange(4999, -1, -1), 2)
    return _coo(rows, rng.integers(0, 5000, len(rows)), 5000, 5000)


def pass_boundary_required_rows(n_rows):
    want = [0, 2047, 2048, n_rows - 1, 2 ** 22 - 1, 2 ** 22]
    return sorted({r for r in want if r < n_rows})


def pass_boundaries(n_rows):
    """6,000 unsorted entries over n_rows either side of one and of two
    11-bit digits (key_max = n_rows - 1), the rows at the digit edges among
    them, each five times."""
    rng = np.random.default_rng(n_rows)
    nnz = 6000
    rows = rng.integers(0, n_rows, nnz)
    must = pass_boundary_required_rows(n_rows)
    at = rng.permutation(np.arange(1, nnz - 1))[:5 * len(must)]
    rows[at] = np.repeat(must, 5)
    rows[0], rows[-1] = n_rows - 1, 0
    return _coo(rows, rng.integers(0, 50, nnz), n_rows, 50)


@functools.lru_cache(maxsize=None)
def scan_carry():
    """2,050 tiles, so 1,025 scan blocks: the block-sum scan takes a second
    step with a carry.  One hub row holds an eighth of the entries."""
    rng = np.random.default_rng(14)
    n, nnz = 70000, SCAN_CARRY_NNZ
    rows = rng.integers(0, n, nnz)
    rows[rng.permutation(nnz)[:nnz // 8]] = 31337
    rows[0], rows[-1] = n - 1, 0
    return _coo(rows, rng.integers(0, n, nnz), n, n)


@functools.lru_cache(maxsize=None)
def plan_scan_carry(last_bin=False):
    """Degrees of 2048 x 2048 + 3 rows for sgc_plan_sorted (descending, two
    passes, 1,025 scan blocks): uniform in [0, 40), three rows of 3,000.
    The counts are digit-major and the scan block past the first 1,024 holds
    digit 2,047 alone, which these degrees never have (3000 - deg is 0 or
    2,961 .. 3,000): the carry is computed there and never used.  last_bin:
    the same with 200 rows of 953 = 3000 - 2047 all over the range, whose
    slots do come from that block."""
    rng = np.random.default_rng(15)
    n = 2048 * 2048 + 3
    deg = rng.integers(0, 40, n)
    deg[[7, n // 2, n - 1]] = 3000
    if last_bin:
        deg[np.linspace(5000, n - 2, 200).astype(np.int64)] = 953
    assert int(deg.sum()) < 2 ** 31
    return deg.astype(np.int64)


def _block_rows(nnz, n_rows=1000):
    return (np.arange(nnz, dtype=np.int64) * n_rows) // nnz


def _cols_in_row(rows):
    """0, 1, 2, ... inside every row of sorted rows."""
    k = np.arange(len(rows))
    first = np.concatenate([[True], rows[1:] != rows[:-1]])
    return k - np.maximum.accumulate(np.where(first, k, 0))


def _swap(case, k):
    rows, cols, vals = case.rows.copy(), case.cols.copy(), case.vals.copy()
    for a in (rows, cols, vals):
        a[k], a[k + 1] = a[k + 1].copy(), a[k].copy()
    assert rows[k] > rows[k + 1]
    return Coo(rows, cols, vals, case.n_rows, case.n_cols)


def wrap_violation(kind):
    """Sorted rows with ascending columns and exactly one fault, which only
    the thread pair across the grid-stride wrap (entries 2,097,151 |
    2,097,152) or across a block edge (255 | 256) sees.
    "wrap" / "block": the two entries swapped (rows no longer sorted; the CSR
    is unchanged and still ascending).  "wrap_equal_columns": no swap, the two
    entries share a row and a column: only bit 2 drops."""
    k = GRID_THREADS - 1
    if kind == "block":
        rows = _block_rows(700)               # 700 entries over rows 0 .. 999, one each
        return _swap(_coo(rows, _cols_in_row(rows), 1000, 8), 255)
    if kind == "wrap":
        # rows 0 .. 998 up to entry k, row 999 from k + 1 on
        rows = np.concatenate([(np.arange(k + 1, dtype=np.int64) * 999) // (k + 1),
                               np.full(WRAP_NNZ - k - 1, 999)])
        return _swap(_coo(rows, _cols_in_row(rows), 1000, 4096), k)
    assert kind == "wrap_equal_columns"
    rows = _block_rows(WRAP_NNZ)
    assert rows[k] == rows[k + 1]
    cols = _cols_in_row(rows)
    cols[k + 1] = cols[k]
    return _coo(rows, cols, 1000, 4096)


def column_major(n_rows=400, n_cols=300):
    """A canonical matrix listed by (col, row), as adj.t() or a column-major
    edge list is: rows unsorted, every CSR row strictly ascending.  The
    status is exactly 2."""
    rng = np.random.default_rng(n_rows)
    flat = rng.choice(n_rows * n_cols, 5000, replace=False)
    r, c = flat // n_cols, flat % n_cols
    o = np.lexsort((r, c))
    return _coo(r[o], c[o], n_rows, n_cols)


def sorted_gaps(n_rows=10000):
    """Sorted rows, canonical: rows 0..99, the last 100 and 5,000 in the
    middle empty.  n_rows = 1: one row; n_rows = 0: nothing at all."""
    rng = np.random.default_rng(16)
    if n_rows == 0:
        return _coo([], [], 0, 5)
    if n_rows == 1:
        return _coo([0] * 4, [0, 2, 3, 6], 1, 7)
    live = np.concatenate([np.arange(100, 2400), np.arange(7400, n_rows - 100)])
    r = rng.choice(live, 9000)
    flat = np.unique(r * 64 + rng.integers(0, 64, len(r)))      # sorted by (row, col), no repeats
    return _coo(flat // 64, flat % 64, n_rows, 64)


def special_value_bits():
    """Unsorted rows whose values are the patterns arithmetic would change:
    NaNs with payloads (quiet and signalling, both signs), +-inf, -0.0,
    denormals."""
    rng = np.random.default_rng(17)
    pat = np.concatenate([
        np.array([0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001, 0x807fffff],
                 np.uint32),
        np.uint32(0x7f800001) + np.arange(40, dtype=np.uint32),      # signalling NaNs
        np.uint32(0x7fc00000) + np.arange(40, dtype=np.uint32),      # quiet NaNs
        np.uint32(0xff800001) + np.arange(40, dtype=np.uint32) * np.uint32(0x1001),
        np.uint32(0xffc00000) + np.arange(40, dtype=np.uint32) * np.uint32(0x0101),
    ])
    assert len(np.unique(pat)) == len(pat)
    rows = rng.integers(0, 20, len(pat))
    rows[0], rows[-1] = 19, 0
    return _coo(rows, rng.integers(0, 30, len(pat)), 20, 30, rng.permutation(pat).view(np.float32))


COO_CASES = {
    **{f"nnz_edges[{n}]": functools.partial(nnz_edges, n) for n in NNZ_EDGES},
    "one_key_many_tiles": one_key_many_tiles,
    "one_key_many_tiles[after_a_later_row]": functools.partial(one_key_many_tiles, True),
    "two_keys_interleaved": two_keys_interleaved,
    "reverse_rows": reverse_rows,
    **{f"pass_boundaries[{n}]": functools.partial(pass_boundaries, n) for n in PASS_BOUNDARY_ROWS},
    "scan_carry": scan_carry,
    **{f"wrap_violation[{k}]": functools.partial(wrap_violation, k)
       for k in ("wrap", "block", "wrap_equal_columns")},
    "column_major[400x300]": functools.partial(column_major, 400, 300),
    "column_major[300x400]": functools.partial(column_major, 300, 400),
    **{f"sorted_gaps[{n}]": functools.partial(sorted_gaps, n) for n in (10000, 1, 0)},
    "special_value_bits": special_value_bits,
}
# more than two million entries: the raw ABI only (once each), and the model
BIG_CASES = ("scan_carry", "wrap_violation[wrap]", "wrap_violation[wrap_equal_columns]")
SMALL_CASES = tuple(n for n in COO_CASES if n not in BIG_CASES)
# the statuses the issue names; every other one is the reference's
EXPECTED_STATUS = {"column_major[400x300]": 2, "column_major[300x400]": 2,
                   "wrap_violation[wrap]": 2, "wrap_violation[block]": 2,
                   "wrap_violation[wrap_equal_columns]": 1, "sorted_gaps[10000]": 3}


def coo_case(name):
    return COO_CASES[name]()


# ---------------------------------------------------------------------------
# inputs the ingest must refuse

def narrowing():
    """{name: Coo} over an 8 x 8 matrix: one index that is out of range as
    int64 and in range once cut to 32 bits, first, last and in the middle."""
    good_r, good_c = [0, 1, 1, 3, 6, 7], [2, 0, 5, 3, 7, 1]
    bad = {"row=2^32+1": (2 ** 32 + 1, 4), "col=2^32": (4, 2 ** 32),
           "row=-2^32": (-2 ** 32, 4), "col=2^31": (4, 2 ** 31)}
    out = {}
    for what, (r, c) in bad.items():
        for where, at in (("first", 0), ("middle", 3), ("last", len(good_r))):
            out[f"{what},{where}"] = _coo(np.insert(good_r, at, r), np.insert(good_c, at, c), 8, 8)
    return out


BAD_CROW_SHAPE = (6, 7)


def valid_small_csr():
    crow = np.array([0, 2, 2, 5, 6, 6, 9], np.int64)
    col = np.array([1, 4, 0, 3, 6, 2, 0, 5, 6], np.int64)
    return crow, col, (np.arange(9) + 1).astype(np.float32)


def bad_crow():
    """{name: (crow, col, vals)}: a valid 6 x 7 CSR of 9 entries with one
    fault each.  nnz stays 9 = len(col): nothing is read past an array."""
    crow, col, vals = valid_small_csr()
    nnz = len(col)

    def with_(a, k, v):
        b = a.copy()
        b[k] = v
        return b
    return {
        "crow[0]=1": (with_(crow, 0, 1), col, vals),
        "crow[-1]=nnz-1": (with_(crow, -1, nnz - 1), col, vals),
        "crow[-1]=nnz+1": (with_(crow, -1, nnz + 1), col, vals),
        "interior_decrease": (with_(crow, 3, 1), col, vals),      # 0 2 2 [1] 6 6 9, all in [0, nnz]
        "crow[2]=-1": (with_(crow, 2, -1), col, vals),
        "crow[3]=2^32": (with_(crow, 3, 2 ** 32), col, vals),
        "col=2^32+1": (crow, with_(col, 4, 2 ** 32 + 1), vals),
    }


# ---------------------------------------------------------------------------
# csrc/sort.hip as written, in numpy

DIGIT_BITS = 11
BINS = 1 << DIGIT_BITS
WAVE = 64                    # pairs ranked by one ballot
PER_WAVE = 512               # consecutive pairs of one wave
TILE = 4 * PER_WAVE          # pairs per count / scatter block
SCAN_BLOCK = 4096            # counts per scan block
SUMS_STEP = 1024             # block sums per step of the one-block scan
UNWRITTEN_KEY, UNWRITTEN_VAL = np.uint32(0xffffffff), np.int32(-1)

MUTANTS = {
    "a": "the rank inside a 64-pair chunk is taken in reverse lane order",
    "b": "wave bases within a tile are not prefixed: all four waves start at the tile's offset",
    "c": "the block-sum scan drops its carry after the first 1,024 blocks",
    "d": "one pass too few for key_max exactly 2^11 or 2^22",
    "e": "the digit mask is kBins instead of kBins - 1",
    "f": "with three passes, the second pass writes the buffer it reads",
    "g": "descending order uses ~key instead of key_max - key",
    "h": "descending order uses -key instead of key_max - key",
}
# (g) changes no result: key <= key_max < 2^(11 * passes), so the digits the
# passes look at are those of 2^(11 * passes) - 1 - key, which falls as key
# rises exactly as key_max - key does, ties in input order either way.  No
# input can tell the two apart and the cases do not try; the descending
# mutant that is a fault is (h), which sorts key 0 first.
EQUIVALENT_MUTANTS = ("g",)
# which case catches which mutant (each of these must; others may)
KILLED_BY = {
    "a": ("nnz_edges[63]", "two_keys_interleaved", "one_key_many_tiles[after_a_later_row]",
          "plan_small"),
    "b": ("nnz_edges[513]", "one_key_many_tiles", "two_keys_interleaved"),
    "c": ("scan_carry", "plan_scan_carry[last_bin]"),
    "d": ("pass_boundaries[2049]", f"pass_boundaries[{2 ** 22 + 1}]"),
    "e": ("nnz_edges[2]", "reverse_rows", "plan_small"),
    "f": (f"pass_boundaries[{2 ** 22 + 1}]",),
    "h": ("plan_small",),
}


class ModelFault(Exception):
    """The modelled kernel would write outside its output."""


def _digit(keys, key_max, desc, shift, mutant):
    if not desc:
        k = keys
    elif mutant == "g":
        k = ~keys
    elif mutant == "h":
        k = np.uint32(0) - keys
    else:
        k = np.uint32(key_max) - keys
    mask = BINS if mutant == "e" else BINS - 1
    return ((k >> np.uint32(shift)) & np.uint32(mask)).astype(np.int64)


def _exclusive_scan(counts, mutant):
    """scan_blocks_kernel, scan_sums_kernel, scan_add_kernel."""
    m = len(counts)
    nb = -(-m // SCAN_BLOCK)
    a = np.zeros(nb * SCAN_BLOCK, np.uint32)
    a[:m] = counts
    a = a.reshape(nb, SCAN_BLOCK)
    inc = np.cumsum(a, axis=1, dtype=np.uint32)
    sums = inc[:, -1].copy()
    a = inc - a
    carry = np.uint32(0)
    for c0 in range(0, nb, SUMS_STEP):
        part = sums[c0:c0 + SUMS_STEP]
        inc_part = np.cumsum(part, dtype=np.uint32)
        total = inc_part[-1]
        sums[c0:c0 + SUMS_STEP] = carry + (inc_part - part)
        carry = np.uint32(0) if mutant == "c" else np.uint32(carry + total)
    a += sums[:, None]
    return a.reshape(-1)[:m]


def _offsets(d, n_tiles, mutant):
    """radix_count_kernel + the scan: first slot of every (digit, tile),
    digit-major.  (A digit past the bins, mutant e, lengthens the arrays
    here where the kernel would leave its own.)"""
    bins = max(BINS, int(d.max()) + 1)
    tile = np.arange(len(d)) // TILE
    counts = np.bincount(d * n_tiles + tile, minlength=bins * n_tiles).astype(np.uint32)
    return _exclusive_scan(counts, mutant), bins


def _since(start):
    k = np.arange(len(start))
    return k - np.maximum.accumulate(np.where(start, k, 0))


def _pass(src_k, src_v, dst_k, dst_v, key_max, desc, shift, mutant):
    """One digit pass into another buffer, every pair at once.  A pair's slot
    is its (digit, tile) offset + the pairs of its digit in the waves before
    its own + those in its wave's chunks before its own + its rank among
    the lanes of its chunk."""
    n = len(src_k)
    n_tiles = -(-n // TILE)
    d = _digit(src_k, key_max, desc, shift, mutant)
    offsets, _ = _offsets(d, n_tiles, mutant)
    tile = np.arange(n) // TILE
    group = tile * (2 * BINS) + d
    o = np.argsort(group, kind="stable")             # by (tile, digit), input order inside
    g = group[o]
    new_group = np.concatenate([[True], g[1:] != g[:-1]])
    new_wave = new_group | np.concatenate([[True], (o[1:] // PER_WAVE) != (o[:-1] // PER_WAVE)])
    new_chunk = new_wave | np.concatenate([[True], (o[1:] // WAVE) != (o[:-1] // WAVE)])
    in_tile, in_wave, in_chunk = _since(new_group), _since(new_wave), _since(new_chunk)
    if mutant == "a":
        starts = np.flatnonzero(new_chunk)
        size = np.diff(np.concatenate([starts, [n]]))
        in_chunk_rank = np.repeat(size, size) - 1 - in_chunk
    else:
        in_chunk_rank = in_chunk
    waves_before = 0 if mutant == "b" else in_tile - in_wave
    chunks_before = in_wave - in_chunk
    pos = np.empty(n, np.int64)
    pos[o] = offsets[d[o] * n_tiles + tile[o]] + waves_before + chunks_before + in_chunk_rank
    if pos.max() >= n:
        raise ModelFault("scatter past the output")
    dst_k[pos] = src_k
    dst_v[pos] = src_v


def _pass_stepwise(src_k, src_v, dst_k, dst_v, key_max, desc, shift, mutant):
    """The same pass as the kernels step through it: the count over the whole
    input first, then tile after tile, per-wave next-slot counters, 64 pairs
    at a time.  Also right when dst is src (a pass that overwrites its own
    input, tiles taken in order), which _pass cannot express."""
    n = len(src_k)
    n_tiles = -(-n // TILE)
    offsets, bins = _offsets(_digit(src_k, key_max, desc, shift, mutant), n_tiles, mutant)
    offsets = offsets.reshape(bins, n_tiles)
    for t in range(n_tiles):
        lo = t * TILE
        base = np.zeros((4, bins), np.int64)
        run = offsets[:, t].astype(np.int64)
        for w in range(4):
            part = src_k[lo + w * PER_WAVE:min(n, lo + (w + 1) * PER_WAVE)]
            base[w] = run
            if mutant != "b":
                run = run + np.bincount(_digit(part, key_max, desc, shift, mutant), minlength=bins)
        for w in range(4):
            for s in range(lo + w * PER_WAVE, min(n, lo + (w + 1) * PER_WAVE), WAVE):
                ck, cv = src_k[s:s + WAVE].copy(), src_v[s:s + WAVE].copy()
                cd = _digit(ck, key_max, desc, shift, mutant)
                pos = np.zeros(len(ck), np.int64)
                todo = np.ones(len(ck), bool)
                while todo.any():               # one digit of the chunk per turn, lowest lane first
                    dl = cd[np.flatnonzero(todo)[0]]
                    same = np.flatnonzero(cd == dl)
                    rank = np.arange(len(same))
                    pos[same] = base[w, dl] + (rank[::-1] if mutant == "a" else rank)
                    base[w, dl] += len(same)
                    todo[same] = False
                if pos.max() >= n:
                    raise ModelFault("scatter past the output")
                dst_k[pos] = ck
                dst_v[pos] = cv


def radix_sort_model(keys, key_max, descending=False, mutant=None, stepwise=False):
    """radix_sort_pairs(keys, 0..n-1): (keys_out, vals_out).  Slots no pass
    wrote keep UNWRITTEN_KEY / UNWRITTEN_VAL."""
    keys = np.ascontiguousarray(keys).astype(np.uint32)
    n = len(keys)
    out_k, out_v = np.full(n, UNWRITTEN_KEY), np.full(n, UNWRITTEN_VAL)
    if n == 0:
        return out_k, out_v
    key_max = int(key_max)
    bit_count = max(0, key_max - 1).bit_length() if mutant == "d" else key_max.bit_length()
    passes = max(1, -(-bit_count // DIGIT_BITS))
    tmp_k, tmp_v = np.full(n, UNWRITTEN_KEY), np.full(n, UNWRITTEN_VAL)
    src_k, src_v = keys, np.arange(n, dtype=np.int32)
    for p in range(passes):
        to_out = (passes - 1 - p) % 2 == 0          # the last pass writes the output
        dst_k, dst_v = (out_k, out_v) if to_out else (tmp_k, tmp_v)
        if mutant == "f" and passes == 3 and p == 1:
            dst_k, dst_v = src_k, src_v
        step = _pass_stepwise if stepwise or dst_k is src_k else _pass
        step(src_k, src_v, dst_k, dst_v, key_max, descending, p * DIGIT_BITS, mutant)
        src_k, src_v = dst_k, dst_v
    return out_k, out_v


def model_coo_to_csr(case, mutant=None, stepwise=False):
    """The unsorted branch of sgc_coo_to_csr on the model: sort (row,
    position), gather, row_ptr from the sorted keys."""
    keys, perm = radix_sort_model(case.rows, max(0, case.n_rows - 1), False, mutant, stepwise)
    row_ptr = np.searchsorted(keys, np.arange(case.n_rows + 1), side="left").astype(np.int32)
    if len(keys) and not np.all(np.diff(keys.astype(np.int64)) >= 0):
        row_ptr = None                               # (row_ptr_from_sorted_kernel needs sorted keys)
    return row_ptr, case.cols[perm].astype(np.int32), case.vals[perm]


def model_plan_sorted(deg, mutant=None, stepwise=False):
    """sgc_plan_sorted's order: rows by degree, longest first, ties ascending."""
    deg = np.asarray(deg, np.int64)
    return radix_sort_model(deg, deg.max() if len(deg) else 0, True, mutant, stepwise)[1]


def plan_small():
    """Degrees 0 .. 40 over 5,000 rows (one pass, descending, three tiles)."""
    return np.random.default_rng(18).integers(0, 41, 5000).astype(np.int64)


PLAN_CASES = {"plan_scan_carry": plan_scan_carry,
              "plan_scan_carry[last_bin]": functools.partial(plan_scan_carry, True),
              "plan_small": plan_small}
BIG_PLAN_CASES = ("plan_scan_carry", "plan_scan_carry[last_bin]")
