"""Operands and a numpy model for the fused training step on 16-bit features
(csrc/xent16.hip: sgc_linear_xent_x16), built on tests/classifier_probes_x16.py.

Launch A of that step, xent_fwd_x16_kernel, has no logits output.  Two kinds
of operands let the public outputs (loss, dW, db) speak for its logits and its
softmax all the same:

* the single-term step: a window of rows each holding ONE full-mantissa 16-bit
  element in a column of its own, so z[m, c] = x_m * W[c, k_m] is one product
  and dW[:, k_m] = x_m * G[m, :] is one term: M * dW[:, k_m] / x_m is row m of
  launch A's G = softmax(z) - onehot, and a logit that lost one of the
  split-bf16 products moves it;
* the softmax-edge step: test_fused_xent_softmax_edges's construction with
  amplitudes that are exact in bf16 and fp16 -- every logit is one exact product
  plus the bias, so the fp32 logits are known on the CPU and the reference is
  the fp64 cross-entropy of exactly them.

`model_step` is launch A in numpy -- logits by x16_product_model (and its
drop-one-product mutants), the epilogue in fp32 as the kernel writes it, the
per-tile double partial -- followed by launch B's single-term products; its
epilogue mutants are the ways the re-laid softmax could be wrong.
`check_single_term` and `check_edge` are the verdicts of the GPU tests
(tests/test_gpu_xent_x16_edges.py); tests/test_xent_x16_probes_cpu.py applies
them to the model and shows each mutant failing a named case.

Plain numpy + torch on the CPU; no GPU, no native library.
"""
import functools

import numpy as np
import torch

import classifier_probes as cp
import classifier_probes_x16 as p16
from adam_ref import FLOOR

F_ = torch.nn.functional
DTYPES = p16.DTYPES
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}

EPILOGUE_MUTANTS = ("no_max", "lse_then_subtract", "max_per_lane_group", "pad_classes_in_sum",
                    "rows_past_M_in_loss")

# tests/test_gpu_xent_x16.py's tolerances against fp64 (loss; dW and db)
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)
# test_fused_xent_softmax_edges's: loss as above, db, and dW per column scaled by max |x|
EDGE_DB_TOL = dict(rtol=1e-4, atol=1e-7)
EDGE_DW_RTOL, EDGE_DW_ATOL = 1e-4, 1e-7
# a drop-one-product mutant must stand this far above the single-term bound
MUTANT_MARGIN = 8.0

OFFSETS = (0.0, 1000.0, -1000.0, 30000.0, -30000.0)
EDGE_K = 16
EDGE_AMPS = (1.0, 1.0, 256.0, 8192.0, 0.0)  # by m % 5: two randn rows, lead 256, lead 8192, flat


def past_workgroups(n_cus=256):
    """tests/test_gpu_xent_x16.py's past_workgroups() for a device of n_cus
    compute units (an MI355X has 256): more 16-row tiles than workgroups."""
    return 16 * (n_cus + 3) + 5


# ---- the single-term step -------------------------------------------------------

# (M, K, C, r0); M = None stands for past_workgroups() and r0 = None for M - 64
SINGLE_TERM_CASES = [(48, 64, 17, 0), (37, 66, 41, 0), (48, 130, 48, 0), (129, 64, 17, 5),
                     (None, 64, 17, None)]
# a small-C shape: the weak mutants (hl, mm) do not clear the margin there
SMALL_C_CASE = (16, 16, 3, 0)


def single_term_seed(M, K, C, r0):
    return cp.single_term_seed(M, K, C) + 31 * r0


class Probe(dict):
    """A dict whose keys read as attributes."""
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def single_term_step(M, K, C, r0, seed, dtype):
    """X [M, K] `dtype`, zero but for one element per row of the window
    [r0, r0 + n), n = min(K, M - r0): row r0 + i holds x[i] (full mantissa,
    |x| in [1, 4)) in column cols[i], the columns distinct.  W [C, K] fp32 full
    mantissa, |w| in [0.5, 4); no bias (b = 0).  Labels of the window cycle
    through the row's largest logit, its smallest and a random class; the
    other rows (all logits 0) get random ones.

    References in fp64 from the exact products z64[i, c] = x[i] * W[c, cols[i]]:
    G64 = softmax(z64) - onehot [n, C] (not divided by M), loss64 (the mean
    over all M rows; a row outside the window contributes log C) and db64 =
    sum_m G / M (a row outside the window 1 / C - onehot)."""
    n = min(K, M - r0)
    assert 0 <= r0 and n >= 1
    g = torch.Generator().manual_seed(seed)
    x = p16.full_mantissa_x16(g, (n,), dtype, emin=0, emax=2)
    W = cp.full_mantissa(g, (C, K), emin=-1, emax=2)
    cols = torch.randperm(K, generator=g)[:n]
    rows = torch.arange(r0, r0 + n)
    X = torch.zeros((M, K), dtype=dtype)
    X[rows, cols] = x
    z64 = x.double()[:, None] * W.double()[:, cols].t()  # exact: 11 + 24 bits
    y = torch.randint(0, C, (M,), generator=g)
    pick = torch.arange(n) % 3
    y[rows] = torch.where(pick == 0, z64.argmax(1), torch.where(pick == 1, z64.argmin(1), y[rows]))
    onehot = F_.one_hot(y, C).double()
    G64 = torch.softmax(z64, 1) - onehot[rows]
    outside = torch.ones(M, dtype=torch.bool)
    outside[rows] = False
    loss_rows = torch.logsumexp(z64, 1) - z64[torch.arange(n), y[rows]]
    n_out = int(outside.sum())
    loss64 = (loss_rows.sum() + n_out * torch.log(torch.tensor(float(C), dtype=torch.float64))) / M
    db64 = (G64.sum(0) + (1.0 / C - onehot[outside]).sum(0)) / M
    return Probe(M=M, K=K, C=C, r0=r0, n=n, dtype=dtype, X=X, W=W, y=y, rows=rows, cols=cols,
                 x=x.double(), z64=z64, G64=G64, loss64=loss64, db64=db64)


def single_term_error(probe, dW):
    """(e, stray): e = max |M * dW[:, k_m] / x_m - G64[m, :]| over the window's
    rows and the classes -- row m of launch A's G as the step's public dW shows
    it, against fp64; stray: whether a column no window row owns is non-zero
    (every term of it is a product with a zero x: it must be exactly 0)."""
    dW = torch.as_tensor(dW).double().cpu()
    got = probe.M * dW[:, probe.cols].t() / probe.x[:, None]
    e = float((got - probe.G64).abs().max())
    other = torch.ones(probe.K, dtype=torch.bool)
    other[probe.cols] = False
    return e, bool((dW[:, other] != 0).any())


def _close(got, ref, rtol, atol):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def check_single_term(probe, got, e32):
    """The GPU test's verdict on got = (loss, dW, db) of a step on the probe:
    (e, failures).  e32 is the same measure of the fp32 step on X.float();
    failures names what missed: "e" (e > 2 e32 + FLOOR), "stray", "loss", "db"
    (tests/test_gpu_xent_x16.py's tolerances against fp64)."""
    loss, dW, db = got
    e, stray = single_term_error(probe, dW)
    bad = []
    if not e <= 2 * e32 + FLOOR:
        bad.append("e")
    if stray:
        bad.append("stray")
    if not _close(loss, probe.loss64, **LOSS_TOL):
        bad.append("loss")
    if not _close(db, probe.db64, **GRAD_TOL):
        bad.append("db")
    return e, bad


# ---- the softmax-edge step ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def softmax_edge_step(M, C, seed):
    """test_fused_xent_softmax_edges's rows with amplitudes exact in bf16 and
    fp16: K = 16, X[m] = a e_k with a = 1, 1, 256, 8192, 0 by m mod 5; k < 8
    picks a 3 randn column of W, k >= 8 a column that is 1 at one random class
    and 0 elsewhere (that class then leads by a); a zero row has all logits
    equal.  The offset comes through the bias (edge_case)."""
    g = torch.Generator().manual_seed(seed)
    K = EDGE_K
    W = torch.zeros((C, K))
    W[:, :8] = torch.randn((C, 8), generator=g) * 3
    lead_cls = torch.randint(0, C, (8,), generator=g)
    W[lead_cls, torch.arange(8, 16)] = 1.0
    kind = torch.arange(M) % 5
    col = torch.where(kind < 2, torch.randint(0, 8, (M,), generator=g),
                      torch.randint(8, 16, (M,), generator=g))
    amp = torch.tensor(EDGE_AMPS)[kind]
    X = torch.zeros((M, K))
    X[torch.arange(M), col] = amp
    for dt in DTYPES:
        assert torch.equal(X.to(dt).float(), X)
    y_rand = torch.randint(0, C, (M,), generator=g)
    return Probe(M=M, K=K, C=C, X=X, W=W, kind=kind, col=col, amp=amp, y_rand=y_rand)


def edge_seed(M, C):
    return 7 * M + C


EDGE_LABELS = ("turns", "lead")


def edge_case(probe, off, bias=True, labels="turns"):
    """The edge problem at a common offset `off` (through the bias; bias=False:
    no bias at all, off must be 0): b, the labels -- on the spread rows the
    leading class or the smallest logit by turns ("turns") or the leading
    class throughout ("lead"), random otherwise -- the fp32 logits z32 =
    fl(a W[:, k] + b) (a is a power of two or zero, so the product is exact
    and the sum is rounded once) and the fp64 cross-entropy of exactly those:
    loss, G = (softmax - onehot) / M, db = sum_m G, dW = G^T X.

    Why "lead" exists: a label on the smallest logit of a row that leads by
    256 or 8192 costs that much, so under "turns" the mean loss is about 850
    and its tolerance (rtol 1e-5) about 8e-3 -- wider than half an ulp of
    30000 (2^-10), which is all a loss formed as (max + log sum) - z_y loses.
    Under "lead" the loss is of order 1 and that rounding shows."""
    M, C = probe.M, probe.C
    assert bias or off == 0.0
    assert labels in EDGE_LABELS
    b = torch.full((C,), float(off))
    prod = probe.X.double() @ probe.W.double().t()
    assert torch.equal(prod.float().double(), prod)  # one exact product each
    z32 = (prod + b.double()).float()                 # RNE of the exact sum
    zk = z32.double()
    m = torch.arange(M)
    y = zk.argmax(1)
    if labels == "turns":
        y = torch.where(m % 2 == 0, y, zk.argmin(1))
    y = torch.where(probe.kind < 2, probe.y_rand, y)
    loss = F_.cross_entropy(zk, y)
    G = (torch.softmax(zk, 1) - F_.one_hot(y, C).double()) / M
    return Probe(off=off, b=b if bias else None, y=y, z32=z32, loss=loss, G=G, db=G.sum(0),
                 dW=G.t() @ probe.X.double())


def edge_variants():
    """(offset, bias, labels) of every call the edge tests make on one
    problem: the five offsets under both label rules, and the offset-0
    problem without a bias."""
    out = [(off, True, lab) for lab in EDGE_LABELS for off in OFFSETS]
    return out + [(0.0, False, "turns")]


def edge_name(M, C, off, bias, labels, dtype):
    return (f"edge M={M} C={C} offset {off:+.0f} labels {labels}{'' if bias else ' no bias'} "
            f"{IDS[dtype]}")


def check_edge(probe, case, got):
    """The GPU test's verdict on got = (loss, dW, db or None): the names of
    what missed among "finite", "loss", "db", "dW" (test_fused_xent_softmax_
    edges's tolerances)."""
    loss, dW, db = got
    outs = [torch.as_tensor(t).double().cpu() for t in (loss, dW) + (() if db is None else (db,))]
    bad = []
    if not all(bool(torch.isfinite(t).all()) for t in outs):
        bad.append("finite")
    if not _close(loss, case.loss, **LOSS_TOL):
        bad.append("loss")
    if db is not None and not _close(db, case.db, **EDGE_DB_TOL):
        bad.append("db")
    room = EDGE_DW_ATOL * probe.X.abs().max(0).values.double()[None, :] + EDGE_DW_RTOL * case.dW.abs()
    if not bool(((outs[1] - case.dW).abs() <= room).all()):
        bad.append("dW")
    return bad


# ---- launch A (and B's single terms) in numpy -----------------------------------

def _row_terms(X):
    """(x [M] fp32, k [M]) of an X with at most one non-zero per row."""
    Xf = X.float().numpy()
    assert ((Xf != 0).sum(1) <= 1).all()
    k = np.abs(Xf).argmax(1)
    return Xf[np.arange(Xf.shape[0]), k], k


def model_logits(X, W, b, dtype, drop=None, exact32=False):
    """Launch A's logits [M, C] fp32 for a one-element-per-row X: the split
    products of x16_product_model (`drop`: one left out), accH + accL, then the
    bias.  exact32: the exact product rounded once instead (what a perfect
    fp32 GEMM gives)."""
    x, k = _row_terms(X)
    w = W.numpy()[:, k].T  # [M, C]
    xe = np.broadcast_to(x[:, None], w.shape)
    if exact32:
        z = (xe.astype(np.float64) * w.astype(np.float64)).astype(np.float32)
    else:
        z = p16.x16_product_model(xe, w, dtype, drop=drop)
    if b is not None:
        z = z + b.numpy().astype(np.float32)[None, :]
    return z.astype(np.float32)


def model_epilogue(z, y, mutant=None, pad_logits=None):
    """xent_fwd_x16_kernel's row epilogue on fp32 logits z [M, C], as the
    kernel writes it: lane (j, kg) of a tile holds row j and classes
    16 n + 4 kg + r; classes >= C are -inf; the maximum and the sum run over
    the lane's classes, then across the four lanes of the row (xor 16, xor
    32); p = exp(z - max) / sum, G = (p - onehot) * (1 / M), the row's loss
    (max - z_y) + log(sum) in fp32; each 16-row tile sums its rows' losses in
    double by a fixed tree (rows past M count 0), the tiles are summed in
    double and scaled by 1 / M.  -> (loss fp32, G [M, C] fp32).

    mutant: no_max (the maximum is not subtracted), lse_then_subtract
    ((max + log sum) - z_y), max_per_lane_group (the maximum is not exchanged
    between the four lanes: classes with equal (c % 16) // 4 use their own, and
    the row's loss lane 0's), pad_classes_in_sum (classes C .. C16 - 1 count
    with z = 0), rows_past_M_in_loss (the missing rows of a ragged last tile
    count as the kernel sees them: their X reads as zero, so their logits are
    pad_logits -- the bias, zero by default -- under the clamped last row's
    label)."""
    assert mutant is None or mutant in EPILOGUE_MUTANTS
    f32 = np.float32
    z = np.ascontiguousarray(z, dtype=f32)
    y = np.asarray(y)
    M_real, C = z.shape
    if mutant == "rows_past_M_in_loss" and M_real % 16:
        extra = 16 - M_real % 16
        row = np.zeros(C, f32) if pad_logits is None else np.asarray(pad_logits, f32)
        z = np.concatenate([z, np.broadcast_to(row, (extra, C))])
        y = np.concatenate([y, np.full(extra, y[-1])])
    M = z.shape[0]
    C16 = (C + 15) // 16 * 16
    zp = np.full((M, C16), 0.0 if mutant == "pad_classes_in_sum" else -np.inf, f32)
    zp[:, :C] = z
    counted = np.zeros(C16, bool)
    counted[:C16 if mutant == "pad_classes_in_sum" else C] = True
    kg = (np.arange(C16) % 16) // 4
    with np.errstate(all="ignore"):
        mx_lane = np.stack([zp[:, kg == q].max(1) for q in range(4)], 1)  # [M, 4]
        mx_row = mx_lane.max(1)
        if mutant == "no_max":
            mx_cls = np.zeros((M, C16), f32)
            mx_loss = np.zeros(M, f32)
        elif mutant == "max_per_lane_group":
            mx_cls = mx_lane[:, kg]
            mx_loss = mx_lane[:, 0]
        else:
            mx_cls = np.broadcast_to(mx_row[:, None], (M, C16))
            mx_loss = mx_row
        ez = np.where(counted[None, :], np.exp((zp - mx_cls).astype(f32)).astype(f32), f32(0))
        lane = []
        for q in range(4):  # the lane's classes in the order n, r
            s = np.zeros(M, f32)
            for c in np.nonzero(kg == q)[0]:
                s = (s + ez[:, c]).astype(f32)
            lane.append(s)
        se = ((lane[0] + lane[1]).astype(f32) + (lane[2] + lane[3]).astype(f32)).astype(f32)
        ls = np.log(se).astype(f32)
        p = (ez[:, :C] / se[:, None]).astype(f32)
        onehot = np.zeros((M, C), f32)
        onehot[np.arange(M), y] = 1
        inv_m = f32(1.0) / f32(M_real)
        G = ((p - onehot).astype(f32) * inv_m).astype(f32)
        zy = z[np.arange(M), y]
        if mutant == "lse_then_subtract":
            row_loss = ((mx_loss + ls).astype(f32) - zy).astype(f32)
        else:
            row_loss = ((mx_loss - zy).astype(f32) + ls).astype(f32)
        n_tiles = (M + 15) // 16
        part = np.zeros(n_tiles * 16, np.float64)
        part[:M] = row_loss
        part = part.reshape(n_tiles, 16)
        for o in (1, 2, 4, 8):  # l += shfl_xor(l, o)
            part = part + part[:, np.arange(16) ^ o]
        total = 0.0
        for t in part[:, 0]:
            total = total + t
        loss = f32(total * (1.0 / M_real))
    return loss, G[:M_real]


def model_step(X, W, b, y, dtype, drop=None, mutant=None, exact32=False):
    """The whole step on a one-element-per-row X: model_logits, model_epilogue,
    then dW[c, k] = the sum over the rows that own column k of launch B's
    split product float(x_m) * G[m, c] (x16_product_model; one term where the
    column has one owner) and db = the fp32 sum of G's rows.
    -> (loss, dW [C, K], db [C]) as torch tensors."""
    z = model_logits(X, W, b, dtype, drop=drop, exact32=exact32)
    loss, G = model_epilogue(z, y.numpy(), mutant=mutant,
                             pad_logits=None if b is None else b.numpy())
    x, k = _row_terms(X)
    with np.errstate(all="ignore"):
        term = p16.x16_product_model(np.broadcast_to(x[:, None], G.shape), G, dtype)
        dW = np.zeros((W.shape[0], W.shape[1]), np.float64)
        np.add.at(dW.T, k, term.astype(np.float64))
        db = G.sum(0, dtype=np.float32)
    return (torch.tensor(float(loss), dtype=torch.float32), torch.from_numpy(dW.astype(np.float32)),
            torch.from_numpy(db))
