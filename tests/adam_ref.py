"""fp64 restatements for the Adam tests: `ref_adam_step` (the element update
include/sgc_amd.h documents, torch.optim.Adam's default single-tensor math),
its mutants, `ref_train` (the citation loop with closed-form gradients) and
the inputs the GPU one-step test and the host mutant test share.

`adam_math` is written with operators only, so the same text runs on fp64 or
fp32 torch tensors (any device) and on numpy arrays."""
import math

import numpy as np
import torch

BETAS = (0.9, 0.999)
EPS = 1e-8
FLOOR = 2.0 ** -22  # tests/test_gpu_lbfgs.py's: four fp32 epsilons

MUTANTS = ("wd_after_moments", "eps_inside_sqrt", "bias_from_step_minus_1", "v_from_raw_g")


def adam_math(p, g, m, v, step, lr, wd, betas=BETAS, eps=EPS, mutant=None):
    """-> (p, m, v) after Adam step `step` (the count after the update)."""
    b1, b2 = betas
    g0 = g
    if wd != 0 and mutant != "wd_after_moments":
        g = g + wd * p
    m = m + (g - m) * (1 - b1)
    gv = g0 if mutant == "v_from_raw_g" else g
    v = b2 * v + (1 - b2) * gv * gv
    t = step - 1 if mutant == "bias_from_step_minus_1" else step
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    with np.errstate(all="ignore"):
        step_size = lr / bc1 if bc1 != 0 else math.inf
        if mutant == "eps_inside_sqrt":
            denom = (v + eps) ** 0.5 / (math.sqrt(bc2) if bc2 > 0 else 0.0)
        else:
            denom = v ** 0.5 / (math.sqrt(bc2) if bc2 > 0 else 0.0) + eps
        upd = m / denom
        if wd != 0 and mutant == "wd_after_moments":
            upd = upd + wd * p
        p = p - step_size * upd
    return p, m, v


def ref_adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, wd, betas=BETAS, eps=EPS,
                  mutant=None):
    """One step on lists of fp64 tensors; a None gradient skips its tensor
    (returned unchanged).  -> (params, exp_avgs, exp_avg_sqs), new lists."""
    out = ([], [], [])
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        r = (p, m, v) if g is None else adam_math(p, g, m, v, step, lr, wd, betas, eps, mutant)
        for o, x in zip(out, r):
            o.append(x)
    return out


def xent_grads(X, W, b, y):
    """loss, dW, db of mean cross-entropy(X W^T + b, y) in the inputs' dtype."""
    M = X.shape[0]
    z = X @ W.t()
    if b is not None:
        z = z + b
    mx = z.max(1, keepdim=True).values
    ez = (z - mx).exp()
    se = ez.sum(1, keepdim=True)
    rows = torch.arange(M, device=X.device)
    loss = ((mx[:, 0] - z[rows, y]) + se[:, 0].log()).mean()
    G = ez / se
    G[rows, y] -= 1.0
    G = G / M
    return loss, G.t() @ X, (G.sum(0) if b is not None else None)


def ref_train(X, W, b, y, epochs, lr, wd, step0=0, state=None, betas=BETAS, eps=EPS):
    """The loop of citation.py:44-50 in fp64.  state: (mW, vW, mb, vb) or None
    (zeros).  -> dict(W, b, mW, vW, mb, vb, loss=[epochs])."""
    X, W = X.double(), W.double()
    b = None if b is None else b.double()
    if state is None:
        state = (torch.zeros_like(W), torch.zeros_like(W),
                 None if b is None else torch.zeros_like(b),
                 None if b is None else torch.zeros_like(b))
    mW, vW, mb, vb = (None if s is None else s.double() for s in state)
    losses = []
    for e in range(epochs):
        loss, dW, db = xent_grads(X, W, b, y)
        losses.append(loss)
        W, mW, vW = adam_math(W, dW, mW, vW, step0 + e + 1, lr, wd, betas, eps)
        if b is not None:
            b, mb, vb = adam_math(b, db, mb, vb, step0 + e + 1, lr, wd, betas, eps)
    return dict(W=W, b=b, mW=mW, vW=vW, mb=mb, vb=vb, loss=torch.stack(losses))


def rel_err(x, x64):
    """tests/test_gpu_lbfgs.py's measure: |x - x64| / |x64| in fp64 (an
    all-zero reference: the absolute error)."""
    x64 = x64.double().cpu()
    d = (x.double().cpu() - x64).norm()
    n = x64.norm()
    return float(d / n) if float(n) > 0 else float(d)


# --- the one-step cases (GPU test and host mutant test) ---------------------------------

SIZES = (1, 63, 64, 65, 1023, 1025, 4097)
LR = 0.2


def one_step_case(n, step, wd, edge=None, seed=0):
    """fp32 CPU tensors (p, g, m, v): a state `step - 1` reference steps would
    plausibly have left, rounded to fp32.  edge: None, "zero_grad",
    "tiny_grad" (|g| = 1e-12, zero moments: eps dominates) or "subnormal_v"."""
    gen = torch.Generator().manual_seed(1000 * seed + n)
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    if step == 1:
        m, v = torch.zeros_like(p), torch.zeros_like(p)
    else:
        m = 0.3 * torch.randn(n, generator=gen, dtype=torch.float64)
        v = 0.5 * torch.rand(n, generator=gen, dtype=torch.float64) + 1e-3
    if edge == "zero_grad":
        g = torch.zeros_like(g)
    elif edge == "tiny_grad":
        g = 1e-12 * torch.where(g >= 0, 1.0, -1.0).double()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
    elif edge == "subnormal_v":
        g = torch.zeros_like(g)
        v = 1e-40 * (1.0 + torch.rand(n, generator=gen, dtype=torch.float64))
        m = 1e-20 * torch.randn(n, generator=gen, dtype=torch.float64)
    return tuple(t.float() for t in (p, g, m, v))


ONE_STEP_CASES = [(n, step, wd, None) for n in SIZES for step, wd in ((1, 0.0), (10000, 5e-4))] + \
    [(1025, 1, 5e-4, None), (1025, 10000, 0.0, None)] + \
    [(1025, step, wd, edge) for edge in ("zero_grad", "tiny_grad", "subnormal_v")
     for step, wd in ((1, 0.0), (10000, 5e-4))]


def one_step_errors(case, run):
    """run(p, g, m, v, step, wd) -> (p, m, v) in any dtype; -> its rel_err
    against the fp64 restatement per output, on the case's fp32 inputs."""
    n, step, wd, edge = case
    p, g, m, v = one_step_case(n, step, wd, edge)
    ref = adam_math(p.double(), g.double(), m.double(), v.double(), step, LR, wd)
    got = run(p, g, m, v, step, wd)
    return {k: rel_err(torch.as_tensor(x), r) for k, x, r in zip("pmv", got, ref)}
