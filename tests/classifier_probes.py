"""Operands that make the classifier kernels' results checkable exactly.

The classifier (linear.hip, xent.hip, loss.hip) is otherwise tested against
fp64 torch on randn data with tolerances that scale with the largest output.
Two kinds of operands remove the tolerance:

* integer operands: every product and every partial sum is an integer below
  2^24, so fp32 arithmetic is exact in any summation order and a correct
  kernel equals the fp64 result bit for bit;
* single-term operands: each output is one product of two full-mantissa
  values (or exactly zero), so its error is one kernel's rounding alone:
  2^-24 for an fp32 product, at most 1.5 * 2^-24 for the split-bf16 scheme
  of csrc/split_bf16.h.

`split3` and `split_product_model` are a numpy model of that scheme (and of
its one-product-missing mutants); tests/test_classifier_probes_cpu.py uses it
to show that the bound the GPU tests apply (2^-22) separates the intact
scheme from every mutant on exactly the single-term data.

Plain numpy + torch on the CPU; no GPU, no native library.
"""
import numpy as np
import torch

EXACT_LIMIT = float(2 ** 24)  # integers below it are exact in fp32
FP32_BOUND = 2.0 ** -23       # one rounded product, twice its rounding
SPLIT_BOUND = 2.0 ** -22      # split-bf16: 2^-24 (final add) + < 2^-24 (dropped ml, lm, ll)

PRODUCTS = ("hh", "hm", "mh", "hl", "lh", "mm")  # x piece, w piece; the kernels' order


# ---- the split-bf16 scheme, in numpy ------------------------------------------

def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; finite x."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """(h, m, l), each a bf16 value held in fp32, with h + m + l == x exactly:
    h = RNE(x), m = RNE(x - h), l = RNE(x - h - m) (split_bf16.h)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r = x - h  # exact (Sterbenz)
    m = bf16_rne(r)
    lo = bf16_rne(r - m)
    return h, m, lo


def split_product_model(x, w, drop=None, mm_as_ml=False):
    """Elementwise x * w as the split kernels form a single-term dot product:
    hh into one fp32 accumulator, the five small products into another in the
    kernels' order (hm, mh, hl, lh, mm), the two added once.  `drop` names a
    product left out (a mutant); `mm_as_ml` pairs x's m with w's l in place of
    m with m (the mutant that reads the wrong piece)."""
    assert drop is None or drop in PRODUCTS
    px = dict(zip("hml", split3(x)))
    pw = dict(zip("hml", split3(w)))
    acc_h = np.zeros(np.shape(x), np.float32)
    acc_l = np.zeros(np.shape(x), np.float32)
    for name in PRODUCTS:
        if name == drop:
            continue
        a, b = px[name[0]], pw[name[1]]
        if name == "mm" and mm_as_ml:
            b = pw["l"]
        p = a * b  # two 8-bit significands: exact in fp32
        if name == "hh":
            acc_h = acc_h + p
        else:
            acc_l = acc_l + p  # fp32 add, rounded like the MFMA's accumulate
    return acc_h + acc_l


def rel_err(got, ref):
    """|got - ref| / |ref| in fp64 (ref non-zero)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.abs(ref)


# ---- integer operands ---------------------------------------------------------

# bits -> (largest |wide value|, smallest "large" wide value, largest |narrow value|)
_INT_MODES = {8: (255, 1, 255), 10: (1023, 256, 7), 18: (262143, 131072, 3)}
_BIAS_MAX = 1000


def _piece_abs(t):
    """|h| + |m| + |l| per element: what a split kernel's partial sums can
    reach (1023 = 1024 - 1 has pieces of total magnitude 1025)."""
    h, m, lo = split3(t.numpy())
    return torch.from_numpy(np.abs(h).astype(np.float64) + np.abs(m) + np.abs(lo))


def integer_bound(A, B, bias=None):
    """max over outputs of sum_k |a||b| (+ |bias|) for A [R, L], B [S, L] (the
    dot products run over L), with every value replaced by the total
    magnitude of its bf16 pieces: below 2^24 every partial sum of every
    kernel, fp32 or split, is an exact integer."""
    s = _piece_abs(A) @ _piece_abs(B).t()
    if bias is not None:
        s = s + bias.double().abs()[None, :]
    return float(s.max())


def _signed(g, shape, lo, hi):
    mag = torch.randint(lo, hi + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(torch.float32)


def integer_operands(M, K, C, bits, seed, backward=False, wide="x"):
    """Signed-integer fp32 operands: (X [M, K], W [C, K], b [C]) for the
    forward, (X [M, K], dY [M, C]) with backward=True.

    bits = 8:  both operands at most 8-bit integers: only the h piece of the
               bf16 split is non-zero;
    bits = 10: the `wide` operand ("x", or "w" -- W or dY) at most 10 bits, the
               other at most 3: h and m pieces;
    bits = 18: wide at most 18 bits, narrow at most 2, dot products of at most
               40 terms: all three pieces (a 17-bit integer has only two: RNE
               leaves a signed remainder, so h and m cover 8 + 1 + 8 bits).
    The dot products run over K (forward) or M (backward).  Where the full
    ranges would pass 2^24 the magnitudes shrink: for bits = 8 both caps, for
    10 / 18 the share of wide entries that are "large" (>= 2^8 / 2^17, the
    ones with a second / third piece; the rest are below 16).  The bound
    (integer_bound) is asserted, so exactness in fp32 holds in any order."""
    wide_max, large_min, narrow_max = _INT_MODES[bits]
    L = M if backward else K
    if bits == 18:
        assert L <= 40, "18-bit operands: dot products of at most 40 terms"
    g = torch.Generator().manual_seed(seed)
    n_out = C
    shape_x, shape_o = (M, K), ((M, C) if backward else (C, K))
    shape_w, shape_n = (shape_x, shape_o) if wide == "x" else (shape_o, shape_x)
    budget = EXACT_LIMIT - (0 if backward else _BIAS_MAX) - 1
    if bits == 8:
        cap = int(min(255, (budget / L) ** 0.5))
        assert cap >= 1
        Wd = _signed(g, shape_w, 0, cap)
        Nr = _signed(g, shape_n, 0, cap)
    else:
        # mean |wide| ~ p * (large_min + wide_max) / 2 + (1 - p) * 8, mean |narrow| ~
        # narrow_max / 2; aim at a quarter of the budget for the mean dot
        # product's sum of magnitudes
        per_term = budget / 4 / L / (narrow_max / 2)
        p = min(1.0, max(0.0, (per_term - 8) / ((large_min + wide_max) / 2 - 8)))
        assert p * L >= 1, f"no room for a large entry per dot product (L = {L})"
        large = _signed(g, shape_w, large_min, wide_max)
        small = _signed(g, shape_w, 0, 15)
        pick = torch.rand(shape_w, generator=g) < p
        Wd = torch.where(pick, large, small)
        Nr = _signed(g, shape_n, 0, narrow_max)
    X, O = (Wd, Nr) if wide == "x" else (Nr, Wd)
    if backward:
        bound = max(integer_bound(O.t().contiguous(), X.t().contiguous()),
                    float(_piece_abs(O).sum(0).max()))
        assert bound < EXACT_LIMIT, (M, K, C, bits, bound)
        return X, O
    b = _signed(g, (n_out,), 0, _BIAS_MAX)
    bound = integer_bound(X, O, b)
    assert bound < EXACT_LIMIT, (M, K, C, bits, bound)
    return X, O, b


# ---- single-term operands -----------------------------------------------------

def full_mantissa(g, shape, emin=-20, emax=20):
    """fp32 values of random sign, exponent in [emin, emax) and 23 random
    mantissa bits with the lowest set: every one has a non-zero third bf16
    piece, and no piece comes near the subnormals."""
    mant = torch.randint(0, 1 << 23, shape, generator=g, dtype=torch.int64) | 1
    expo = torch.randint(emin, emax, shape, generator=g, dtype=torch.int64) + 127
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64)
    bits = (sign << 31) | (expo << 23) | mant
    return torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy())


def single_term_forward(M, K, C, seed):
    """(X [M, K], W [C, K], x [M], ref [M, C] fp64): X[m, :] is zero but for
    x[m] at column m mod K, so Y[m, c] = x[m] * W[c, m mod K] is one product;
    ref is that product in fp64 (exact: 48 bits)."""
    g = torch.Generator().manual_seed(seed)
    x = full_mantissa(g, (M,))
    W = full_mantissa(g, (C, K))
    X = torch.zeros((M, K))
    rows = torch.arange(M)
    X[rows, rows % K] = x
    ref = x.double()[:, None] * W.double()[:, rows % K].t()
    return X, W, x, ref


def single_term_backward(M, K, C, r0, seed):
    """(X, dY, dYb, wref, wbref, bref) for the weight backward.  X as in
    single_term_forward.  dY [M, C] is full-mantissa on the rows
    [r0, min(r0 + K, M)) and zero elsewhere: each column k of X meets at most
    one of those rows, so dW[c, k] = dY[m, c] * x[m] is one product (wref,
    fp64) or exactly zero.  dYb keeps one element of dY per class (class c in
    row r0 + c mod rows): db of dYb is that element (bref, fp32), and dW of
    dYb (wbref) has one non-zero per class."""
    g = torch.Generator().manual_seed(seed)
    x = full_mantissa(g, (M,))
    X = torch.zeros((M, K))
    rows = torch.arange(M)
    X[rows, rows % K] = x
    r1 = min(r0 + K, M)
    assert 0 <= r0 < r1
    dY = torch.zeros((M, C))
    dY[r0:r1] = full_mantissa(g, (r1 - r0, C))
    dYb = torch.zeros((M, C))
    cls = torch.arange(C)
    at = r0 + cls % (r1 - r0)
    dYb[at, cls] = dY[at, cls]
    wref = torch.zeros((C, K), dtype=torch.float64)
    blk = rows[r0:r1]
    wref[:, blk % K] = dY[r0:r1].double().t() * x[r0:r1].double()[None, :]
    wbref = torch.zeros((C, K), dtype=torch.float64)
    wbref[cls, at % K] = dYb[at, cls].double() * x[at].double()
    bref = dYb[at, cls].clone()
    return X, dY, dYb, wref, wbref, bref


def check_single_term(got, ref, bound):
    """(largest relative error over ref's non-zero elements in units of 2^-24,
    ok): elements whose expected value is zero must be exactly zero, the
    others within `bound` relative."""
    got = got.double()
    zero = ref == 0
    err = ((got - ref).abs() / ref.abs().masked_fill(zero, 1.0)).masked_fill(zero, 0.0)
    worst = float(err.max())
    ok = bool((got[zero] == 0).all()) and worst <= bound
    return worst * 2.0 ** 24, ok


# ---- the cases of tests/test_gpu_classifier_exact.py ----------------------------
# (kept here so the CPU suite checks the generators at the very shapes the GPU
# tests use)

def case_seed(M, K, C):
    return 1000003 * M + 1009 * K + C


def single_term_seed(M, K, C):
    return case_seed(M, K, C) + 7


# Integer forward: (M, K, C, ld_extra, bits, wide, kernels, auto).  ld_extra:
# NaN columns behind X's K.  kernels: t = the LDS tile (tile_buffers 1 and 2),
# s = the fp32 streaming kernel (linear_ck 32 and 64; it needs an even row
# pitch: K + ld_extra a multiple of 4 gives 16-B loads, else 8-B loads),
# p = the split-bf16 kernel (W's three images must fit LDS: K <= 416 at 64
# classes).  auto: the kernel the automatic choice must name (M >= 4096), or
# None.  M = 70,000 gives a wave more than one tile on 256 CUs; C > 64 runs a
# second class block (of 1, 6 and 64 + 1 classes).
FORWARD_CASES = [
    (1, 1, 1, 1, 8, "x", "tsp", None),
    (15, 3, 15, 1, 18, "x", "tsp", None),         # pitch 4: 16-B loads
    (17, 31, 16, 0, 18, "w", "tp", None),         # odd pitch: 4-B aligned rows
    (33, 33, 17, 1, 18, "x", "tsp", None),        # pitch 34: 8-B loads
    (129, 63, 41, 1, 10, "x", "tsp", None),       # pitch 64
    (257, 65, 42, 1, 10, "w", "tsp", None),       # pitch 66
    (129, 130, 48, 2, 10, "x", "tsp", None),      # pitch 132
    (257, 130, 49, 0, 10, "w", "tsp", None),      # pitch 130; a fourth class tile of 1
    (33, 333, 64, 1, 10, "x", "tsp", None),       # pitch 334; four full class tiles
    (17, 333, 65, 6, 8, "x", "tp", None),         # split: second class block of 1
    (129, 130, 70, 2, 10, "w", "tsp", None),      # split: second class block of 6
    (257, 63, 129, 0, 8, "x", "tp", None),        # three class blocks
    (4099, 602, 41, 2, 10, "x", "tsp", "linear_split_kernel"),   # pitch 604: 16-B
    (4099, 602, 48, 0, 10, "w", "ts", "linear_stream_kernel"),   # W's split image > LDS
    (4099, 602, 49, 0, 10, "x", "t", "linear_kernel"),           # neither image fits
    (70000, 602, 41, 0, 10, "x", "tsp", "linear_split_kernel"),  # pitch 602: 8-B
    (70000, 63, 17, 1, 8, "w", "sp", "linear_split_kernel"),     # pitch 64: 16-B
]

# Integer backward: (M, K, C, ldx_extra, ldd_extra, bits, wide, kernels).
# kernels: the kernel that backward_kernel = 0, 1, 2, 3 must name, c = the
# split-bf16 column blocks (up to 48 classes), f = the fp32 slabs, s = the
# split-bf16 slabs (K and X's pitch even).  The Ms, per kernel:
#   column blocks (48 row ranges x 4 waves x 32-row steps): 33 = 2 steps, fewer
#     than ranges, the second of one row; 6145 = 193 steps, every wave of every
#     range busy and range 0's wave 0 twice, the last step of one row; 12321 =
#     386 steps, waves 0 (and 1 in ranges 0, 1) take a second trip whose
#     look-ahead load lies past the end;
#   fp32 slabs (slabs of 4-row steps, a ring of 4 in flight): 37 = one slab of
#     10 steps: two turns of the ring, two tail steps, the last of one row;
#     257 / 513 = 2 / 3 slabs, the last shorter and ending in a one-row step;
#     K = 602 gives a wave a second pass over its column groups;
#   split-bf16 slabs (224-row slabs of 32-row steps, 32-column groups, wave w
#     takes groups w, w + 4, ...): 33 / 37 = two steps, the second ragged;
#     257 = a second slab of two steps, the last of one row; K = 130 = five
#     groups, wave 0 a second pass over a group of two columns.
# Ks: the last 64-column block partial (1, 3, 34, 63, 65, 130, 602) or full
# (64), K not a multiple of 4.  Cs: one to three class tiles of the column
# blocks (16 / 17, 32 / 33, 48), their 8- and 12-byte lane loads straddling C
# (17, 33 do not, 41 does: classes 39-41), the fall-back above 48.
BACKWARD_CASES = [
    (33, 1, 1, 1, 0, 8, "x", "cffc"),
    (33, 3, 2, 0, 1, 18, "w", "cffc"),
    (37, 34, 16, 0, 0, 18, "x", "cfsc"),
    (37, 63, 17, 1, 3, 18, "w", "cffc"),
    (33, 602, 41, 0, 0, 18, "x", "cfsc"),
    (257, 64, 32, 0, 0, 10, "x", "cfsc"),
    (257, 65, 33, 3, 1, 10, "w", "cffc"),
    (257, 130, 41, 2, 7, 10, "x", "cfsc"),
    (513, 602, 48, 0, 0, 10, "w", "cfsc"),
    (513, 602, 49, 2, 1, 8, "x", "ffsf"),
    (513, 130, 64, 0, 0, 10, "x", "ffsf"),
    (6145, 602, 41, 0, 0, 10, "x", "cfsc"),
    (6145, 34, 2, 0, 2, 10, "w", "cfsc"),
    (12321, 602, 17, 2, 3, 10, "w", "cfsc"),
    (12321, 65, 33, 1, 0, 8, "x", "cffc"),
]

# Single-term probes: (K, C); the forward takes M = 2 K + 1 (every k position
# hit, rows wrap), the backward M in {K, 6145} with the dY block first, in the
# middle and last (partial).
SINGLE_TERM_SHAPES = [(33, 17), (130, 41), (602, 17), (602, 41)]


def single_term_backward_cases():
    out = []
    for (K, C) in SINGLE_TERM_SHAPES:
        out.append((K, K, C, 0))
        for r0 in (0, 3001, 6145 - (K // 2 + 1)):
            out.append((6145, K, C, r0))
    return out


# ---- slices of wider, NaN-padded tensors ----------------------------------------

def nan_padded(t, extra, device=None):
    """(view, whole): `view` equals t and is the first t.shape[1] columns of a
    tensor `extra` columns wider whose padding holds NaN."""
    whole = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), dtype=t.dtype)
    whole[:, :t.shape[1]] = t
    if device is not None:
        whole = whole.to(device)
    return whole[:, :t.shape[1]], whole
