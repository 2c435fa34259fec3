"""Operands, references and a numpy model for the evaluation kernels
(csrc/eval.hip, eval16.hip: sgc_linear_eval_f32 / _x16).

* Exact problems: small-integer X, W and b, so every logit is an integer below
  2^24 -- exact in fp32 in any summation order and in every bf16 split -- and
  the expected prediction is the first-maximum argmax of the int64 logits.
  `exact_operands` takes tests/classifier_probes.py's integer operands;
  `tie_operands` plants exact ties (identical W rows and biases) and makes the
  tied pair the row's two largest logits in every other row.
* `argmax_model` / `count_model`: the kernels' reductions in numpy -- a scan in
  the lane, then a pairwise merge across the lane groups -- with the mutants
  the tests must catch.
* Random problems: the issue's generator, the fp64 reference and the
  decided-row rule.

Plain numpy + torch on the CPU; no GPU, no native library.
"""
import functools

import numpy as np
import torch

import classifier_probes as cp
import classifier_probes_x16 as cpx

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
SGC_DTYPE = {torch.bfloat16: 1, torch.float16: 2}

MUTANTS = ("last_on_tie", "nan_ignored", "ge_across_groups", "padded_may_win", "rows_past_m")


# ---- the argmax rule and the counting, as the kernels reduce them -----------------

def _gt(a, b):
    """a beats b by value alone: torch's order, NaN above everything."""
    an, bn = np.isnan(a), np.isnan(b)
    if an or bn:
        return bool(an and not bn)
    return bool(a > b)


def _eq(a, b):
    return bool(a == b) or bool(np.isnan(a) and np.isnan(b))


def argmax_model(Z, C=None, mutant=None):
    """Row argmax of Z [M, CP] over the classes < C (CP - C padded columns,
    which a correct kernel never lets win), reduced the way eval_fwd_x16_kernel
    does: lane group kg scans its classes 16 n + 4 kg + r in order and keeps the
    first maximum, then the four groups merge pairwise (kg ^ 1, then kg ^ 2) on
    (value, index): the larger value, on equal values the smaller index.
    Mutants: "last_on_tie" keeps the last maximum of the scan; "nan_ignored"
    reads a NaN as -inf (what a reduction on fmaxf does); "ge_across_groups" merges with
    >= on the value alone; "padded_may_win" scans the padded columns too."""
    assert mutant in (None,) + MUTANTS
    Z = np.asarray(Z, dtype=np.float32)
    M, CP = Z.shape
    C = CP if C is None else C
    if mutant == "nan_ignored":
        Z = np.where(np.isnan(Z), np.float32(-np.inf), Z)
    limit = CP if mutant == "padded_may_win" else C
    out = np.zeros(M, dtype=np.int64)
    for m in range(M):
        best = []  # per lane group: (value, index) or None
        for kg in range(4):
            cur = None
            for n in range((CP + 15) // 16):
                for r in range(4):
                    c = 16 * n + 4 * kg + r
                    if c >= limit or c >= CP:
                        continue
                    v = Z[m, c]
                    if cur is None:
                        cur = (v, c)
                    elif _gt(v, cur[0]) or (mutant == "last_on_tie" and
                                                     _eq(v, cur[0])):
                        cur = (v, c)
            best.append(cur)

        def merge(a, b):  # lane a takes lane b's pair when b is better
            if b is None:
                return a
            if a is None:
                return b
            if mutant == "ge_across_groups":
                return b if (_gt(b[0], a[0]) or _eq(b[0], a[0])) else a
            if _gt(b[0], a[0]) or (_eq(b[0], a[0]) and b[1] < a[1]):
                return b
            return a

        step1 = [merge(best[kg], best[kg ^ 1]) for kg in range(4)]
        step2 = [merge(step1[kg], step1[kg ^ 2]) for kg in range(4)]
        out[m] = step2[0][1]
    return out


def count_model(labels, pred, C, mutant=None):
    """(confusion [C, C], counts [2]) as eval_count_kernel forms them: a row
    whose label lies outside [0, C) is left out.  The "rows_past_m" mutant
    also counts the rows between M and the next multiple of 16 (the rest of the
    last tile), which read as label 0 and prediction 0."""
    labels = np.asarray(labels, dtype=np.int64)
    pred = np.asarray(pred, dtype=np.int64)
    if mutant == "rows_past_m":
        pad = (-len(labels)) % 16
        labels = np.concatenate([labels, np.zeros(pad, np.int64)])
        pred = np.concatenate([pred, np.zeros(pad, np.int64)])
    ok = (labels >= 0) & (labels < C)
    y, p = labels[ok], pred[ok]
    cm = np.bincount(y * C + p, minlength=C * C).reshape(C, C).astype(np.int64)
    return cm, np.array([ok.sum(), (y == p).sum()], dtype=np.int64)


# ---- exact problems ------------------------------------------------------------------

def exact_operands(M, K, C, dtype, seed):
    """(X [M, K] in `dtype`, W [C, K], b [C]): classifier_probes' 8-bit integer
    operands (exact in bf16 and fp16 as well; the 2^24 bound is asserted
    there)."""
    if dtype == torch.float32:
        return cp.integer_operands(M, K, C, 8, seed)
    return cpx.integer_operands_x16(M, K, C, 8, seed, dtype)


def tie_operands(M, K, C, dtype, pair, seed):
    """Integer operands with an exact tie planted between the classes of
    `pair` (identical W rows and biases), or between all classes (pair =
    "all": W = 0, b = 0).  X in [-4, 4], W in [-8, 8], b in [-16, 16]; column 0
    of X is 1 in the odd rows and 0 in the even ones, and the tied pair's
    W[:, 0] is 2^20 (0 for every other class): in the odd rows the pair holds
    the two largest logits, exactly equal, so the smaller index must win."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-4, 5, (M, K), generator=g).to(torch.float32)
    W = torch.randint(-8, 9, (C, K), generator=g).to(torch.float32)
    b = torch.randint(-16, 17, (C,), generator=g).to(torch.float32)
    if pair == "all":
        W.zero_()
        b.zero_()
    else:
        c1, c2 = pair
        assert 0 <= c1 < c2 < C
        X[:, 0] = (torch.arange(M) % 2).to(torch.float32)
        W[:, 0] = 0.0
        W[c2] = W[c1]
        b[c2] = b[c1]
        W[c1, 0] = W[c2, 0] = float(2 ** 20)
    assert cp.integer_bound(X, W, b) < cp.EXACT_LIMIT
    X16 = X.to(dtype)
    assert torch.equal(X16.float(), X)
    return X16, W, b


def int_logits(X, W, b):
    """The exact logits as int64 numpy [M, C]."""
    Z = X.double().numpy().astype(np.int64) @ W.double().numpy().astype(np.int64).T
    return Z + b.double().numpy().astype(np.int64)[None, :]


def loss_fp64(Z, labels):
    """mean_m logsumexp(Z_m) - Z[m, y_m] in fp64 (numpy)."""
    Z = np.asarray(Z, dtype=np.float64)
    mx = Z.max(1)
    lse = mx + np.log(np.exp(Z - mx[:, None]).sum(1))
    return float(np.mean(lse - Z[np.arange(len(labels)), labels]))


def labels_for(M, C, seed):
    return torch.from_numpy(np.random.default_rng(seed + 99).integers(0, C, M))


# shapes M x K x C of the exact problems, with the layouts each runs in:
# "c" contiguous, "p" padded pitch (two NaN columns behind K), "w" an offset
# window (rows from 5, columns from 2 of a wider NaN-filled tensor)
EXACT_SHAPES = [
    (1, 64, 1, "c"),
    (15, 64, 2, "c"),
    (16, 66, 17, "c"),
    (17, 130, 48, "c"),
    (37, 66, 41, "cpw"),
    (129, 64, 17, "w"),
    (4149, 66, 17, "c"),    # past the 4096-row threshold of `linear`, ragged last tile
    (4149, 602, 41, "c"),
]
EXACT_SHAPES_FP32 = [(37, 66, 64, "c"), (4149, 130, 64, "c")]  # a fourth class tile


def tie_pairs(C):
    """The planted ties that exist at C classes: (0, 1); (3, 4), the 4 kg + r
    edge; (15, 16), the class-tile edge; (c, C - 1); every class."""
    pairs = [p for p in ((0, 1), (3, 4), (15, 16)) if p[1] < C]
    if C // 2 < C - 1 and (C // 2, C - 1) not in pairs:
        pairs.append((C // 2, C - 1))
    return pairs + ["all"]


def laid_out(X, layout, device):
    """X on `device` in the named layout; the view equals X."""
    M, K = X.shape
    if layout == "c":
        return X.to(device).contiguous()
    if layout == "p":
        return cp.nan_padded(X, 2, device)[0]
    assert layout == "w"
    whole = torch.full((M + 9, K + 6), float("nan"), dtype=X.dtype)
    whole[5:5 + M, 2:2 + K] = X
    return whole.to(device)[5:5 + M, 2:2 + K]


# ---- random problems -----------------------------------------------------------------

RANDOM_SHAPES = [(4149, 66, 17), (4149, 66, 41), (4149, 130, 48), (1000, 602, 41), (4149, 66, 7)]
RANDOM_SEEDS = (0, 1, 2, 3, 4)
UNDECIDED_SHARE = 0.005


@functools.lru_cache(maxsize=None)
def random_problem(M, K, C, seed, dtype):
    """(X in `dtype`, W, b, Zref fp64 numpy, tol): X = standard_normal, W and
    b = 0.1 standard_normal, rounded to the operand types; Zref the fp64 logits
    of the rounded operands; tol = 1e-5 max |Zref|."""
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(dtype)
    W = torch.from_numpy((0.1 * rng.standard_normal((C, K))).astype(np.float32))
    b = torch.from_numpy((0.1 * rng.standard_normal(C)).astype(np.float32))
    Z = X.double().numpy() @ W.double().numpy().T + b.double().numpy()[None, :]
    return X, W, b, Z, 1e-5 * float(np.abs(Z).max())


def decided_rows(Z, tol):
    """Rows whose fp64 top-two gap exceeds 8 tol (C = 1: every row)."""
    if Z.shape[1] == 1:
        return np.ones(len(Z), dtype=bool)
    top = np.sort(Z, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > 8 * tol


def check_random(pred, Z, tol):
    """(undecided rows, wrong decided rows, undecided rows whose class lies
    more than 8 tol below the maximum)."""
    pred = np.asarray(pred)
    dec = decided_rows(Z, tol)
    ref = Z.argmax(1)
    wrong = int((pred[dec] != ref[dec]).sum())
    und = ~dec
    rows = np.nonzero(und)[0]
    far = int((Z[rows].max(1) - Z[rows, pred[rows]] > 8 * tol).sum())
    return int(und.sum()), wrong, far
