"""Operands that take the SpMM's FMA chains through every IEEE edge.

The propagation is bit-identical with torch.spmm on the CPU: per output
element one sequential fmaf chain in storage order, starting from +0.0f.  On
aug-normalised S and randn X every intermediate of that chain is an ordinary
normal number, and several kinds of kernel error change nothing there: one FMA
too many with a zero weight (fma(0, x, acc) == acc unless acc is -0.0 or x is
not finite), flushed subnormals, a first product taken by a multiply.  The
operands built here make those errors visible on every row length the
kernels treat differently.

edge_graph     a raw (not normalised) CSR with strictly ascending columns:
               row lengths over the kernels' edges, three long rows that meet
               the special nodes only at chosen positions, one all-negative row
               per length and a long one
edge_coo       the same matrix as a COO with duplicates in shuffled order
big_graph      the same value rules on millions of short rows (one-row kernel's
               whole-block schedule)
edge_features  "wild" (inf, NaN, overflow, subnormals, signed zeros) or "quiet"
               (finite for three hops of the "quiet" graph)
census         what a result holds, per row-length class
compare        the one comparison rule: NaN where the reference is NaN (payload
               and sign free), equal bits everywhere else
fma32 / chain  numpy model of the chain and of its mutants (host tests)

A -0.0 result needs every product of the chain to underflow to -0: exact zero
products give +0.0 from the +0.0 start (+0 + -0 = +0).  So it appears only
where all of a row's S values are negative and small and X is +2^-149 (the
all-negative rows against the first deep-tiny column); a mixed-sign row of
hundreds of nonzeros with |s| up to 2^9 leaves zero at its first normal
product and does not return, so among the long rows the conditions tests ask
the all-negative one for it.

Plain numpy + torch on the CPU; no GPU, no native library.
"""
import functools
from types import SimpleNamespace

import numpy as np

ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 100)
LONG_ROWS = (3001, 900, 300)       # mixed signs; 3001 > one 2880-nonzero hub pass at HC = 32
LONG_NEGATIVE = 3001               # the long all-negative row
PLACED = (0, 63, 64, 239, 240, 479, 480, -1)  # positions of special nodes in a long row
N_SPECIAL = 24
HUGE_NODE_SHARE = 0.03
S_SPECIAL_SHARE = 0.03
S_SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-42, 2.0 ** -126, -2.0 ** -126], np.float32)
X_SPECIALS = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40], np.float32)
CLASS_NAMES = ("empty", "1-4", "5-16", "17-64", "65-100",
               "long3001", "long900", "long300", "longneg")
SHORT_CLASSES = ("1-4", "5-16", "17-64", "65-100")
MIXED_LONG = ("long3001", "long900", "long300")
COUNTS = ("neg_zero", "pos_zero", "subnormal", "pos_inf", "neg_inf", "nan", "normal")


def _row_class(length):
    length = np.asarray(length)
    return np.select([length == 0, length <= 4, length <= 16, length <= 64], [0, 1, 2, 3], 4)


def _pow2_values(rng, size, lo, hi):
    """Random sign, magnitude 2^e * m with integer e in [lo, hi], m in [1, 2):
    one 32-bit draw per element (sign, eight exponent bits, the mantissa), in
    cache-sized pieces."""
    out = np.empty(size, np.float32)
    flat = out.reshape(-1)
    for i in range(0, flat.size, 1 << 18):
        u = rng.integers(0, 1 << 32, min(1 << 18, flat.size - i), dtype=np.uint32)
        e = (u >> np.uint32(23)) & np.uint32(0xFF)
        e *= np.uint32(hi - lo + 1)
        e >>= np.uint32(8)
        u &= np.uint32(0x807FFFFF)
        if lo >= -126:
            e += np.uint32(127 + lo)
            e <<= np.uint32(23)
            u |= e
            flat[i:i + u.size] = u.view(np.float32)
        else:  # subnormals: ldexp rounds +-[1, 2) * 2^e
            u |= np.uint32(0x3F800000)
            flat[i:i + u.size] = np.ldexp(u.view(np.float32), e.astype(np.int32) + np.int32(lo))
    return out


def _ascending_columns(lens, n, rng):
    """Strictly ascending columns for rows of `lens` nonzeros (all < n / 2):
    random steps of at least one, a random offset.  Vectorised."""
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    row = np.repeat(np.arange(lens.size), lens)
    smax = np.maximum(1, n // (lens + 1))
    steps = 1 + (rng.random(row.size) * smax[row]).astype(np.int64)
    c = np.cumsum(steps)
    before = np.concatenate([[0], c])[rp[:-1]]  # the cumulative sum before each row
    c -= before[row]
    last = np.zeros(lens.size, np.int64)
    nz = lens > 0
    last[nz] = c[rp[1:][nz] - 1]
    offset = (rng.random(lens.size) * (n - last + 1)).astype(np.int64)
    col = c - 1 + np.minimum(offset, n - last)[row]
    return rp, col


@functools.lru_cache(maxsize=None)
def hot_nodes(n, seed=0):
    """(special, placed, huge): the special nodes' ids in index order (the
    first 24 laid out for the long rows' chosen positions, n // 100 more at
    random, which only the short rows meet), the ids each long row meets at
    PLACED, and the
    mask of nodes that are huge in the huge columns."""
    rng = np.random.default_rng([seed, n, 1])
    special, placed, taken = [], [], set()
    for r, L in enumerate(LONG_ROWS):
        pos = sorted({p if p >= 0 else L - 1 for p in PLACED if p < L})
        ids, v, prev = [], 11 + 13 * r, -1
        for p in pos:
            gap = p - prev - 1            # plain columns wanted between two placed ones
            v += 1 + (gap * 5 + 3) // 4 + (8 if gap else 0)
            while v in taken:
                v += 1
            ids.append(v)
            taken.add(v)
            prev = p
        assert ids[-1] < n
        placed.append((np.array(pos), np.array(ids)))
        special += ids
    v = n - 40
    while len(special) < N_SPECIAL:
        if v not in taken:
            special.append(v)
            taken.add(v)
        v -= 29
    special = np.array(special, np.int64)
    more = np.setdiff1d(rng.choice(n, n // 100, replace=False), special)
    special = np.concatenate([special, more])
    huge = rng.random(n) < HUGE_NODE_SHARE
    huge[special] = False
    return special, placed, huge


def _placed_row(L, pos, ids, allowed, rng):
    """Ascending columns of a long row that meets ids[i] at position pos[i] and
    otherwise only `allowed` nodes."""
    out, prev_p, prev_v = [], -1, -1
    for p, v in zip(pos, ids):
        want = p - prev_p - 1
        pool = allowed[(allowed > prev_v) & (allowed < v)]
        assert pool.size >= want, (L, p, pool.size, want)
        out.append(np.sort(rng.choice(pool, want, replace=False)))
        out.append(np.array([v]))
        prev_p, prev_v = p, v
    cols = np.concatenate(out)
    assert cols.size == L and np.all(np.diff(cols) > 0)
    return cols


@functools.lru_cache(maxsize=None)
def edge_graph(n=4096, seed=0, kind="wild"):
    """Raw CSR (row_ptr, col_idx, val; int32 / float32), `row_class` per row
    (index into CLASS_NAMES), `negative_rows`, `long_rows`.  "quiet" scales
    every value by 2^-9 (|s| < 1) and is otherwise the same matrix."""
    assert n >= 4096 and kind in ("wild", "quiet")
    rng = np.random.default_rng([seed, n, 2])
    special, placed, huge = hot_nodes(n, seed)
    lens = np.array(ROW_LENGTHS, np.int64)[np.arange(n) % len(ROW_LENGTHS)]
    # long rows and the all-negative rows (one per length from 1 up, one long)
    long_rows = [n // 7 + 1, n // 2 + 3, n - 29]
    long_neg = n // 3 + 40
    for r, L in zip(long_rows, LONG_ROWS):
        lens[r] = L
    lens[long_neg] = LONG_NEGATIVE
    base = len(ROW_LENGTHS) * (n // (3 * len(ROW_LENGTHS)))
    negative_rows = [base + k for k in range(1, len(ROW_LENGTHS))] + [long_neg]
    assert not set(negative_rows[:-1]) & set(long_rows + [long_neg])
    row_class = _row_class(lens)
    for k, r in enumerate(long_rows + [long_neg]):
        row_class[r] = 5 + k
    is_long = np.zeros(n, bool)
    is_long[long_rows + [long_neg]] = True
    rp_s, col_s = _ascending_columns(np.where(is_long, 0, lens), n, rng)
    plain = np.ones(n, bool)
    plain[special] = False
    plain[huge] = False
    allowed = np.nonzero(plain)[0]
    long_cols = {}
    for r, L, (pos, ids) in zip(long_rows, LONG_ROWS, placed):
        long_cols[r] = _placed_row(L, pos, ids, allowed, rng)
    # the all-negative long row also meets the third long row's special nodes
    # (six nodes, six different columns each: +-inf and NaN beside its -0.0)
    long_cols[long_neg] = np.sort(np.concatenate(
        [rng.choice(allowed, LONG_NEGATIVE - placed[2][1].size, replace=False), placed[2][1]]))
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    col = np.empty(rp[-1], np.int64)
    row = np.repeat(np.arange(n), lens)
    short = ~is_long[row]
    col[short] = col_s
    for r, c in long_cols.items():
        col[rp[r]:rp[r + 1]] = c
    val = _pow2_values(rng, col.size, -8, 8)
    swap = rng.random(col.size) < S_SPECIAL_SHARE
    val[swap] = S_SPECIALS[rng.integers(0, S_SPECIALS.size, int(swap.sum()))]
    neg = np.zeros(n, bool)
    neg[negative_rows] = True
    m = neg[row]
    # |s| in [2^-8, 2^-2): with "quiet"'s 2^-9 still far from underflow
    val[m] = -np.abs(_pow2_values(rng, int(m.sum()), -8, -3))
    if kind == "quiet":
        val = (val * np.float32(2.0 ** -9)).astype(np.float32)
    return SimpleNamespace(n=n, row_ptr=rp.astype(np.int32), col_idx=col.astype(np.int32),
                           val=val, row_class=row_class, negative_rows=np.array(negative_rows),
                           long_rows=np.array(long_rows + [long_neg]), lens=lens, kind=kind,
                           seed=seed)


@functools.lru_cache(maxsize=None)
def big_graph(n, seed=0):
    """Raw CSR for the one-row kernel's large-launch schedule: row lengths
    0-8, ~300 rows of 65-300 nonzeros, three of 3001; the value rules of
    edge_graph("wild")."""
    rng = np.random.default_rng([seed, n, 3])
    lens = np.arange(n, dtype=np.int64) % 9
    mid = rng.choice(n, 303, replace=False)
    lens[mid[:300]] = rng.integers(65, 301, 300)
    lens[mid[300:]] = 3001
    rp, col = _ascending_columns(lens, n, rng)
    val = _pow2_values(rng, col.size, -8, 8)
    swap = rng.random(col.size) < S_SPECIAL_SHARE
    val[swap] = S_SPECIALS[rng.integers(0, S_SPECIALS.size, int(swap.sum()))]
    neg = np.repeat(np.arange(n) % 64 == 5, lens)  # every 64th row all negative
    val[neg] = -np.abs(_pow2_values(rng, int(neg.sum()), -8, -3))
    row_class = _row_class(np.minimum(lens, 100))
    return SimpleNamespace(n=n, row_ptr=rp.astype(np.int32), col_idx=col.astype(np.int32),
                           val=val, row_class=row_class, lens=lens, kind="wild", seed=seed)


@functools.lru_cache(maxsize=None)
def edge_coo(n=4096, seed=0, kind="wild"):
    """(rows, cols, vals) of edge_graph with 5 % of the entries stored twice
    (the copy at half the value: same sign) and the storage order shuffled.
    Not coalesced: torch.spmm and the ingest keep each row's storage order."""
    g = edge_graph(n, seed, kind)
    rng = np.random.default_rng([seed, n, 4])
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.row_ptr))
    dup = np.nonzero(rng.random(rows.size) < 0.05)[0]
    r = np.concatenate([rows, rows[dup]])
    c = np.concatenate([g.col_idx.astype(np.int64), g.col_idx[dup].astype(np.int64)])
    v = np.concatenate([g.val, (g.val[dup] * np.float32(0.5)).astype(np.float32)])
    p = rng.permutation(r.size)
    return r[p], c[p], v[p]


def column_groups(g, bounds):
    """g's nonzeros split by column range [bounds[i], bounds[i+1]): one
    (row_ptr, col_idx, val) per range over the same rows, runs in CSR order."""
    rp = np.asarray(g.row_ptr, np.int64)
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    grp = np.searchsorted(np.asarray(bounds), g.col_idx, side="right") - 1
    out = []
    for i in range(len(bounds) - 1):
        m = grp == i
        sub = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(row[m], minlength=n), out=sub[1:])
        out.append((sub.astype(np.int32), g.col_idx[m], g.val[m]))
    return out


def column_kinds(F):
    """Per feature column: 0 ordinary, 1 tiny (f % 5 == 4), 2 huge (f % 7 == 6),
    3 / 4 the two deep-tiny columns (f % 11 == 2 / 7), 5 the +0 column
    (f % 22 == 10)."""
    f = np.arange(F)
    kind = np.zeros(F, np.int64)
    kind[f % 7 == 6] = 2
    kind[f % 5 == 4] = 1
    kind[f % 11 == 2] = 3
    kind[f % 11 == 7] = 4
    kind[f % 22 == 10] = 5
    return kind


# exponent ranges per storage format: ordinary, tiny, the deep-tiny value, huge
RANGES = {"float32": ((-40, 40), (-149, -125), 2.0 ** -149, (100, 127)),
          # bfloat16: fp32's exponents, subnormals down to 2^-133
          "bfloat16": ((-40, 40), (-133, -120), 2.0 ** -133, (100, 127)),
          # float16: subnormals down to 2^-24, 65504 the largest: products with
          # |s| < 2^9 stay below it except against the huge nodes
          "float16": ((-14, 0), (-24, -12), 2.0 ** -24, (8, 15))}


def edge_features(n, F, kind="wild", seed=0, fmt="float32"):
    """X [n, F] float32 for edge_graph / big_graph of the same (n, seed); read
    only (cached up to 65,536 rows).  fmt "bfloat16" / "float16": the same
    column kinds at that format's exponents (see edge_features16)."""
    if n <= 65536:
        return _edge_features_cached(n, F, kind, seed, fmt)
    return _edge_features(n, F, kind, seed, fmt)


def edge_features16(n, F, kind, dtype, seed=0):
    """The features as a torch bfloat16 / float16 tensor: built at the format's
    own exponent ranges, then rounded to it (torch's round to nearest even)."""
    import torch
    fmt = {torch.bfloat16: "bfloat16", torch.float16: "float16"}[dtype]
    return torch.from_numpy(edge_features(n, F, kind, seed, fmt).copy()).to(dtype)


@functools.lru_cache(maxsize=None)
def _edge_features_cached(n, F, kind, seed, fmt):
    X = _edge_features(n, F, kind, seed, fmt)
    X.setflags(write=False)
    return X


def _edge_features(n, F, kind, seed, fmt):
    (o_lo, o_hi), (t_lo, t_hi), deep, (h_lo, h_hi) = RANGES[fmt]
    tiny = np.float32(deep)
    assert kind in ("wild", "quiet")
    rng = np.random.default_rng([seed, n, F, 5])
    special, _, huge = hot_nodes(n, seed)
    ck = column_kinds(F)
    X = _pow2_values(rng, (n, F), o_lo, o_hi)
    t = np.nonzero(ck == 1)[0]
    if t.size:
        T = _pow2_values(rng, (n, t.size), t_lo, t_hi)
        u = rng.integers(0, 10, (n, t.size), dtype=np.uint8)
        T[u == 0] = 0.0
        T[u == 9] = -0.0
        X[:, t] = T
    d = np.nonzero(ck == 3)[0]
    X[:, d] = tiny
    d = np.nonzero(ck == 4)[0]
    if d.size:
        pick = np.array([tiny, -tiny, 0.0, -0.0], np.float32)
        X[:, d] = pick[rng.integers(0, 4, (n, d.size))]
    X[:, ck == 5] = 0.0
    if kind == "wild":
        h = np.nonzero(ck == 2)[0]
        rows = np.nonzero(huge)[0]
        if h.size:
            X[np.ix_(rows, h)] = _pow2_values(rng, (rows.size, h.size), h_lo, h_hi)
        # special node j holds a special value in ordinary column number q when
        # q % 3 == 0 and (q / 3) % 8 == j % 8: every third ordinary column over
        # the nodes, and the eight nodes a long row meets never share a column
        o = np.nonzero(ck == 0)[0]
        q = np.arange(o.size)
        j = np.arange(special.size)
        jj, qq = np.nonzero((q[None, :] % 3 == 0) & ((q[None, :] // 3) % 8 == j[:, None] % 8))
        X[special[jj], o[qq]] = X_SPECIALS[(jj // 8 + 5 * (qq // 24) + jj % 8) % X_SPECIALS.size]
    return X


# ---- what a result holds, and the comparison rule --------------------------------

def _kinds(Y):
    Y = np.ascontiguousarray(Y, np.float32)
    u = Y.view(np.uint32)
    mag = u & np.uint32(0x7FFFFFFF)
    return {"neg_zero": u == np.uint32(0x80000000), "pos_zero": u == 0,
            "subnormal": (mag > 0) & (mag < np.uint32(0x00800000)),
            "pos_inf": u == np.uint32(0x7F800000), "neg_inf": u == np.uint32(0xFF800000),
            "nan": mag > np.uint32(0x7F800000),
            "normal": (mag >= np.uint32(0x00800000)) & (mag < np.uint32(0x7F800000))}


def census(Y, row_classes, names=CLASS_NAMES):
    """{class name: {kind: count, "total": elements}} over the rows of Y."""
    kinds = _kinds(Y)
    out = {}
    for c, name in enumerate(names):
        rows = np.asarray(row_classes) == c
        if not rows.any():
            continue
        out[name] = {k: int(m[rows].sum()) for k, m in kinds.items()}
        out[name]["total"] = int(rows.sum()) * Y.shape[1]
    return out


def census16(Y16, row_classes, names=CLASS_NAMES):
    """census() of a torch bfloat16 / float16 tensor (its own subnormals)."""
    import torch
    Y16 = Y16.detach().cpu().contiguous()
    bits = Y16.view(torch.int16).numpy().view(np.uint16)
    f = Y16.float().numpy()
    tiny = np.float32(torch.finfo(Y16.dtype).tiny)
    kinds = {"neg_zero": bits == 0x8000, "pos_zero": bits == 0,
             "subnormal": (f != 0) & (np.abs(f) < tiny), "pos_inf": f == np.inf,
             "neg_inf": f == -np.inf, "nan": np.isnan(f),
             "normal": np.isfinite(f) & (np.abs(f) >= tiny)}
    out = {}
    for c, name in enumerate(names):
        rows = np.asarray(row_classes) == c
        if rows.any():
            out[name] = {k: int(m[rows].sum()) for k, m in kinds.items()}
            out[name]["total"] = int(rows.sum()) * f.shape[1]
    return out


def mismatches(got, want):
    """Boolean mask of the elements where `got` breaks the rule against `want`
    (float32, or 16-bit patterns given as torch bfloat16 / float16 tensors)."""
    if hasattr(got, "dtype") and not isinstance(got, np.ndarray):  # torch
        import torch
        got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
        assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype)
        if got.dtype == torch.float32:
            got, want = got.numpy(), want.numpy()
        else:
            gn, wn = torch.isnan(got).numpy(), torch.isnan(want).numpy()
            gb, wb = got.view(torch.int16).numpy(), want.view(torch.int16).numpy()
            return (gn != wn) | (~wn & (gb != wb))
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32)))


def compare(got, want, what=""):
    """The comparison rule: isnan masks equal, bit patterns equal everywhere
    else; a NaN's payload and sign are not compared."""
    bad = mismatches(got, want)
    if bad.any():
        idx = np.argwhere(bad)
        first = tuple(int(i) for i in idx[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in "
                             f"{np.unique(idx[:, 0]).size} rows; first at {first}: "
                             f"got {got[first]!r}, want {want[first]!r}")


def nan_patterns(Y):
    """The distinct NaN bit patterns of a float32 array (information only)."""
    u = np.ascontiguousarray(Y, np.float32).view(np.uint32)
    return sorted({f"{int(p):#010x}" for p in np.unique(u[np.isnan(Y)])})


# ---- the chain in numpy, and its mutants ---------------------------------------

def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64, the
    sum is rounded to odd there (two-sum's error decides), and one rounding
    to float32 follows -- 53 >= 2 * 24 + 2 bits make that the single rounding."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
        c = np.asarray(c, np.float32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0)
        bits = s.copy().view(np.int64)
        even = (bits & 1) == 0
        away = (e > 0) == (s > 0)  # the exact sum lies farther from zero than s
        bits = np.where(fix & even, np.where(away, bits | 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


def ftz(x):
    """Subnormals to zero of the same sign."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    sub = (u & np.uint32(0x7F800000)) == 0
    return np.where(sub, u & np.uint32(0x80000000), u).astype(np.uint32).view(np.float32)


def chain(row_ptr, col_idx, val, X, mutant=None):
    """Y = S . X as per-element chains, all rows in step.  mutant: None (the
    contract), "zero_fma" (a trailing fma(0, X[last col], acc) on every row with
    nonzeros), "ftz" (inputs and every FMA result flushed), "mul_first" (the
    first product by a multiply), "unfused" (round(s * x) + acc),
    "reversed" (last nonzero first)."""
    rp = np.asarray(row_ptr, np.int64)
    n, F = rp.size - 1, X.shape[1]
    lens = np.diff(rp)
    val = np.asarray(val, np.float32)
    X = np.asarray(X, np.float32)
    if mutant == "ftz":
        val, X = ftz(val), ftz(X)
    acc = np.zeros((n, F), np.float32)
    order = np.argsort(-lens, kind="stable")
    sorted_lens = lens[order]
    with np.errstate(all="ignore"):
        for k in range(int(lens.max(initial=0))):
            rows = order[:np.searchsorted(-sorted_lens, -k, side="left")]  # lens > k
            at = rp[rows] + (lens[rows] - 1 - k if mutant == "reversed" else k)
            s, x = val[at][:, None], X[col_idx[at]]
            if mutant == "mul_first" and k == 0:
                new = (s * x).astype(np.float32)
            elif mutant == "unfused":
                new = ((s * x).astype(np.float32) + acc[rows]).astype(np.float32)
            else:
                new = fma32(s, x, acc[rows])
            acc[rows] = ftz(new) if mutant == "ftz" else new
        if mutant == "zero_fma":
            rows = np.nonzero(lens > 0)[0]
            acc[rows] = fma32(np.float32(0.0), X[col_idx[rp[rows + 1] - 1]], acc[rows])
    return acc
