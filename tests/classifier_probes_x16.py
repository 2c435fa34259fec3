"""Operands and a numpy model for the classifier on 16-bit features
(csrc/linear16.hip): the counterpart of tests/classifier_probes.py, which it
builds on.

The kernels take bf16 / fp16 X with fp32 W and dY and compute on the exactly
widened elements.  In the split-bf16 scheme a bf16 x is its own single piece
(h = x), an fp16 x exactly two (h = RNE_bf16(x), m = x - h), W and dY three:

  bf16 X: hh into accH; hm, hl into accL            -- nothing dropped, a
          single-term output within FP32_BOUND = 2^-23 (accH exact, one
          rounded add in accL, the final add);
  fp16 X: hh into accH; hm, mh, hl, mm into accL    -- the dropped ml is the
          term the fp32 scheme drops too: SPLIT_BOUND = 2^-22.

`x16_product_model` is that scheme (and its drop-one-product mutants) in
numpy; tests/test_classifier_x16_cpu.py shows which share of the single-term
data each mutant fails its bound on.

Plain numpy + torch on the CPU; no GPU, no native library.
"""
import numpy as np
import torch

import classifier_probes as cp

DTYPES = (torch.bfloat16, torch.float16)
# (x piece, w piece), the kernels' order; the first goes into accH
PRODUCTS = {torch.bfloat16: ("hh", "hm", "hl"), torch.float16: ("hh", "hm", "mh", "hl", "mm")}
MUTANTS = {torch.bfloat16: ("hm", "hl"), torch.float16: ("hm", "mh", "hl", "mm")}
BOUND = {torch.bfloat16: cp.FP32_BOUND, torch.float16: cp.SPLIT_BOUND}
# Every mutant exceeds BOUND on more than half of the single-term elements
# (measured on the CPU over 2^18 elements: bf16 hm 99.99 %, hl 90 %; fp16 hm
# 99.99 %, mh 100 %, hl 85 %, mm 91 %; the intact schemes reach 0.99 and 1.21
# units of 2^-24): test_classifier_x16_cpu.py asserts it.
MUTANT_SHARE = 0.5


def x_pieces(x, dtype):
    """{piece: fp32 array} of 16-bit values x (given widened to fp32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.bfloat16:
        return {"h": x}
    h = cp.bf16_rne(x)
    m = x - h  # exact: 11 significant bits = 8 + 3
    assert np.array_equal(cp.bf16_rne(m), m)
    return {"h": h, "m": m}


def x16_product_model(x, w, dtype, drop=None):
    """Elementwise float(x) * w as the x16 kernels form a single-term dot
    product: hh into one fp32 accumulator, the small products into another in
    the kernels' order, the two added once.  `drop` names a product left out."""
    names = PRODUCTS[dtype]
    assert drop is None or drop in names
    px = x_pieces(x, dtype)
    pw = dict(zip("hml", cp.split3(w)))
    acc_h = np.zeros(np.shape(x), np.float32)
    acc_l = np.zeros(np.shape(x), np.float32)
    for name in names:
        if name == drop:
            continue
        p = px[name[0]] * pw[name[1]]  # two 8-bit significands: exact in fp32
        if name == "hh":
            acc_h = acc_h + p
        else:
            acc_l = acc_l + p  # fp32 add, rounded like the MFMA's accumulate
    return acc_h + acc_l


def full_mantissa_x16(g, shape, dtype, emin=None, emax=None):
    """`dtype` values of random sign with every mantissa bit random and the
    lowest set (bf16: 7 bits, fp16: 10 -- an fp16 value then has a non-zero m
    piece), exponents away from both types' subnormals: [-20, 20) for bf16,
    [-10, 10) for fp16, or [emin, emax) where both are given."""
    nbits, lo, hi = (7, -20, 20) if dtype == torch.bfloat16 else (10, -10, 10)
    assert (emin is None) == (emax is None)
    if emin is not None:
        assert lo <= emin < emax <= hi
    else:
        emin, emax = lo, hi
    mant = torch.randint(0, 1 << nbits, shape, generator=g, dtype=torch.int64) | 1
    expo = torch.randint(emin, emax, shape, generator=g, dtype=torch.int64) + 127
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64)
    bits = (sign << 31) | (expo << 23) | (mant << (23 - nbits))
    f = torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy())
    out = f.to(dtype)
    assert torch.equal(out.float(), f)
    return out


def integer_operands_x16(M, K, C, bits, seed, dtype, backward=False, wide="x"):
    """cp.integer_operands with X in `dtype`, asserted exact there: bf16 holds
    integers up to 256 (bits = 8, or 10 / 18 with wide = "w": X is the narrow
    operand), fp16 up to 2048 (also bits = 10 with wide = "x", which gives X an
    m piece)."""
    ops = cp.integer_operands(M, K, C, bits, seed, backward=backward, wide=wide)
    X = ops[0]
    X16 = X.to(dtype)
    assert torch.equal(X16.float(), X), (dtype, bits, wide)
    return (X16,) + tuple(ops[1:])


def single_term_forward_x16(M, K, C, seed, dtype):
    """cp.single_term_forward's layout with x from full_mantissa_x16:
    (X [M, K] dtype, W [C, K] fp32, ref [M, C] fp64, exact)."""
    g = torch.Generator().manual_seed(seed)
    x = full_mantissa_x16(g, (M,), dtype)
    W = cp.full_mantissa(g, (C, K))
    X = torch.zeros((M, K), dtype=dtype)
    rows = torch.arange(M)
    X[rows, rows % K] = x
    ref = x.double()[:, None] * W.double()[:, rows % K].t()
    return X, W, ref


def single_term_backward_x16(M, K, C, r0, seed, dtype):
    """cp.single_term_backward's layout with x from full_mantissa_x16:
    (X dtype, dY, dYb, wref, wbref, bref)."""
    g = torch.Generator().manual_seed(seed)
    x = full_mantissa_x16(g, (M,), dtype)
    X = torch.zeros((M, K), dtype=dtype)
    rows = torch.arange(M)
    X[rows, rows % K] = x
    r1 = min(r0 + K, M)
    assert 0 <= r0 < r1
    dY = torch.zeros((M, C))
    dY[r0:r1] = cp.full_mantissa(g, (r1 - r0, C))
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


def nan_padded16(t, extra, device=None):
    """cp.nan_padded for a 16-bit tensor: (view, whole)."""
    return cp.nan_padded(t, extra, device)


# ---- the cases of tests/test_gpu_classifier_x16.py -------------------------------
# Forward: (M, K, C, pad, (bits, wide) for bf16, (bits, wide) for fp16, kernel).
# kernel: the name sgc_linear_x16_kernel_name must give for the view --
# "linear_x16_kernel", or "none" with the path that then runs.
FORWARD_CASES = [
    (1, 1, 1, 1, (8, "x"), (8, "x"), "linear_x16_kernel"),
    (15, 3, 15, 1, (18, "w"), (10, "x"), "linear_x16_kernel"),
    (17, 31, 16, 0, (18, "w"), (18, "w"), "none"),       # odd pitch: the copy path
    (33, 33, 17, 1, (10, "w"), (10, "x"), "linear_x16_kernel"),
    (129, 63, 41, 1, (10, "w"), (10, "x"), "linear_x16_kernel"),   # ragged 64-k double chunk
    (257, 65, 42, 1, (8, "x"), (10, "w"), "linear_x16_kernel"),    # one k past a double chunk
    (129, 130, 48, 2, (10, "w"), (10, "x"), "linear_x16_kernel"),
    (33, 333, 64, 1, (10, "w"), (10, "x"), "linear_x16_kernel"),   # four full class tiles
    (17, 333, 65, 5, (8, "x"), (10, "x"), "linear_x16_kernel"),    # a second class block of 1
    (257, 63, 129, 1, (10, "w"), (8, "x"), "linear_x16_kernel"),   # three class blocks
    (4099, 602, 41, 2, (10, "w"), (10, "x"), "linear_x16_kernel"),
    (4099, 602, 49, 0, (8, "x"), (10, "x"), "none"),     # the image exceeds LDS: the upcast path
    (70000, 63, 17, 1, (10, "w"), (10, "x"), "linear_x16_kernel"),  # more than one tile per wave
]

# Backward: (M, K, C, ldx_pad, ldd_pad, bf16 mode, fp16 mode, kernel).
BACKWARD_CASES = [
    (33, 1, 1, 1, 0, (8, "x"), (8, "x"), "xent_dw_cols_x16_kernel"),
    (33, 3, 2, 1, 1, (18, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (37, 34, 16, 0, 0, (18, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (37, 63, 17, 1, 3, (10, "w"), (18, "w"), "xent_dw_cols_x16_kernel"),
    (33, 602, 41, 0, 0, (18, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (257, 64, 32, 0, 0, (10, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (257, 65, 33, 1, 1, (8, "x"), (10, "w"), "xent_dw_cols_x16_kernel"),
    (257, 130, 41, 2, 7, (10, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (513, 602, 48, 0, 0, (10, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (513, 602, 49, 2, 1, (8, "x"), (10, "x"), "none"),   # above 48 classes: the upcast path
    (6145, 602, 41, 0, 0, (10, "w"), (10, "x"), "xent_dw_cols_x16_kernel"),
    (12321, 65, 33, 1, 0, (8, "x"), (10, "w"), "xent_dw_cols_x16_kernel"),
]


def mode_of(case_modes, dtype):
    return case_modes[0] if dtype == torch.bfloat16 else case_modes[1]
