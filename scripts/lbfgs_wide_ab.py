"""TextSGC classifier training, three ways, alternating in one process:

  torch   torch.optim.LBFGS on the reference closure in torch ops
          (downstream/TextSGC/train.py:52-78: a bias-less linear layer,
          nll_loss(log_softmax) + 0.5 * l2 * (W ** 2).sum())
  step    sgc_amd.optim.LBFGS(wide=True).step on that same closure
  fused   sgc_amd.optim.LBFGS(wide=True).run_steps(model, x, y, 3, l2=l2)

on synthetic float32 features at the corpora's shapes, 3 steps of 20
iterations at history 100.  Per side: the median (min .. max) of the wall time
over the repetitions, the optimiser's share (total minus closures consumed
times one closure's own time), iterations and closures consumed, final loss.

    python scripts/lbfgs_wide_ab.py [--reps 5] [--out profiles/lbfgs_wide/ab.log]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("R8-like", 4937, 15362, 8), ("ohsumed-like", 3021, 21557, 23),
          ("R52-like", 5879, 17992, 52), ("20NG-like", 10183, 61603, 20)]
DEV = "cuda:0"
L2 = 5e-4
STEPS = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def final_loss(W, X, y):
    with torch.no_grad():
        return float(F.cross_entropy(F.linear(X, W), y) + 0.5 * L2 * (W ** 2).sum())


def side_torch_ops(cls, X, y, W0, **kw):
    lin = torch.nn.Linear(W0.shape[1], W0.shape[0], bias=False).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W0)
    opt = cls(lin.parameters(), **kw)

    def closure():
        opt.zero_grad()
        out = lin(X).squeeze()
        loss = F.nll_loss(F.log_softmax(out, dim=1), y) + 0.5 * L2 * (lin.weight ** 2).sum()
        loss.backward()
        return loss

    def run():
        for _ in range(STEPS):
            opt.step(closure)
    seconds, _ = timed(run)
    st = opt.state[opt._params[0]]
    one, _ = timed(lambda: [closure() for _ in range(5)])
    return seconds, st["n_iter"], st["func_evals"], one / 5, final_loss(lin.weight, X, y)


def side_fused(X, y, W0):
    from sgc_amd import _lib
    from sgc_amd.optim import LBFGS
    from sgc_amd.textsgc import SGC
    model = SGC(W0.shape[1], W0.shape[0]).to(DEV)
    with torch.no_grad():
        model.W.weight.copy_(W0)
    opt = LBFGS(model.parameters(), wide=True)
    seconds, _ = timed(lambda: opt.run_steps(model, X, y, STEPS, l2=L2))
    if not opt._dev_wide or opt.step_statuses[0] is None:
        raise RuntimeError("the fused wide call was not taken")
    st = opt.state[opt._params[0]]
    # one closure of the fused loop: sgc_linear_xent_f32 on the same operands
    lib = _lib.load()
    M, K = X.shape
    C = W0.shape[0]
    ws = torch.empty(max(1, lib.sgc_linear_xent_workspace(M, K, C)), dtype=torch.uint8, device=DEV)
    loss, dW = torch.empty(1, device=DEV), torch.empty_like(W0, device=DEV)
    W = model.W.weight.data

    def closures():
        for _ in range(5):
            _lib.check(lib.sgc_linear_xent_f32(_lib.ptr(X), X.stride(0), _lib.ptr(W), None,
                                               _lib.ptr(y), M, K, C, _lib.ptr(loss), _lib.ptr(dW),
                                               None, None, 0, _lib.ptr(ws), ws.numel(),
                                               _lib.stream_handle(DEV)), "linear_xent")
    one, _ = timed(closures)
    return seconds, st["n_iter"], st["func_evals"], one / 5, final_loss(W, X, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    args = ap.parse_args()
    from sgc_amd import _lib
    from sgc_amd.optim import LBFGS
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# lbfgs_wide_ab: {STEPS} steps x 20 iterations, history 100, l2 {L2}, "
        f"{args.reps} alternating repetitions, {torch.cuda.get_device_name(0)}")
    for name, M, K, C in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        g = torch.Generator().manual_seed(0)
        try:
            X = (torch.rand(M, K, generator=g) / 8.0).to(DEV)
        except torch.cuda.OutOfMemoryError as e:
            say(f"{name} {M}x{K}x{C}: not run ({e})")
            continue
        y = torch.randint(0, C, (M,), generator=g).to(DEV)
        torch.manual_seed(1)
        W0 = torch.nn.init.xavier_normal_(torch.empty(C, K)).to(DEV)
        sides = {"torch": lambda: side_torch_ops(torch.optim.LBFGS, X, y, W0),
                 "step": lambda: side_torch_ops(LBFGS, X, y, W0, wide=True),
                 "fused": lambda: side_fused(X, y, W0)}
        res = {k: [] for k in sides}
        failed = {}
        for rep in range(args.reps + 1):  # the first round warms up and is dropped
            for k, fn in sides.items():
                if k in failed:
                    continue
                try:
                    r = fn()
                except _lib.SGCError as e:
                    # an argument refusal made before any launch (the closure's
                    # 31-bit offset limits); anything else ends the script
                    if "(code 1)" not in str(e) and "(code 2)" not in str(e):
                        raise
                    failed[k] = str(e)
                    continue
                if rep:
                    res[k].append(r)
        say(f"{name} {M} x {K} x {C} (n = {K * C})")
        for k in sides:
            if k in failed:
                say(f"  {k:6s} not run: {failed[k]}")
                continue
            ts = [r[0] for r in res[k]]
            opt_share = [r[0] - r[2] * r[3] for r in res[k]]
            _, n_iter, evals, one, loss = res[k][-1]
            say(f"  {k:6s} total {statistics.median(ts) * 1e3:9.2f} ms ({min(ts) * 1e3:.2f} .. "
                f"{max(ts) * 1e3:.2f})  optimiser {statistics.median(opt_share) * 1e3:9.2f} ms "
                f"({min(opt_share) * 1e3:.2f} .. {max(opt_share) * 1e3:.2f})  closure "
                f"{one * 1e3:.3f} ms  n_iter {n_iter} closures {evals}  final loss {loss:.6f}")
        del X
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
