"""A/B of the evaluation stage: the literal expression the drivers run against
SGC.evaluate, in one process with the two interleaved:

    python scripts/eval_ab.py [--samples 30] [--rounds 5] [--out profiles/eval/ab.log]

Shapes: the Reddit validation and test sets (23,699 and 55,334 x 602, 41
classes) in float32, bfloat16 and float16; Cora's (500 and 1000 x 1433, 7
classes) in float32.

  (a) the literal expression: f1(model(x), y) at the Reddit shapes
      (drivers/reddit.py), accuracy(model(x), y) read back with float() at
      Cora's (drivers/citation.py) -- the forward's logits, torch's max, the
      host copies and sklearn;
  (b) model.evaluate(x, y).f1() / float(model.evaluate(x, y).accuracy()).
Both are wall-clock times of the whole expression from a synchronised device
to the value on the host, taken alternately (a, b, a, b, ...): the median and
the standard deviation of each side's samples, and whether (b) is faster than
(a) by more than three standard deviations (the larger of the two sides').

The forward launch alone: sgc_linear_eval_f32 / _x16 asked for the predictions
only (launch A, nothing else) against sgc_linear_f32 / sgc_linear_x16 into a
preallocated logits matrix, both called at the raw ABI with preallocated
buffers -- event-timed, 10 back-to-back calls per sample, the two interleaved
per round; `spread` is max - min of the linear launch over the rounds.  The
evaluation launch stores 8 M bytes where the linear launch stores 4 M C.

Every step runs under its own time limit: a step that overruns ends the
process with status 124.
"""
import argparse
import os
import sys
import threading
from contextlib import contextmanager
from time import perf_counter

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import _lib  # noqa: E402
from sgc_amd.classifier_bench import _median_ms  # noqa: E402
from sgc_amd.metrics import accuracy, f1  # noqa: E402
from sgc_amd.models import SGC  # noqa: E402
from sgc_amd.propagate import X16_DTYPES, warmup  # noqa: E402

TYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
CASES = [("reddit-val", 23699, 602, 41, ("float32", "bfloat16", "float16"), "f1"),
         ("reddit-test", 55334, 602, 41, ("float32", "bfloat16", "float16"), "f1"),
         ("cora-val", 500, 1433, 7, ("float32",), "accuracy"),
         ("cora-test", 1000, 1433, 7, ("float32",), "accuracy")]


@contextmanager
def step_limit(seconds, what):
    """End the process (status 124) if the step takes longer than `seconds`."""
    def overrun():
        print(f"eval_ab: step '{what}' passed its {seconds} s limit", flush=True)
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with step_limit(a.step_limit, "warm-up"):
        warmup(dev)
    say(f"evaluation A/B: {a.samples} alternating samples per side (wall clock, us); the forward "
        f"launch alone: {a.rounds} rounds x {a.reps} reps x 10 calls (events, us)")
    for (case, M, K, C, types, metric) in CASES:
        g = torch.Generator(device="cpu").manual_seed(0)
        x32 = torch.randn(M, K, generator=g)
        teacher = torch.randn(C, K, generator=g) / K ** 0.5
        y = (x32 @ teacher.t() + 0.5 * torch.randn(M, C, generator=g)).argmax(1).to(dev)
        torch.manual_seed(0)
        model = SGC(K, C).to(dev)
        with torch.no_grad():
            model.W.weight.copy_(teacher)
        model.eval()
        W, b = model.W.weight.detach(), model.W.bias.detach()
        for name in types:
            x = x32.to(TYPES[name]).to(dev)

            if metric == "f1":
                def literal():
                    with torch.no_grad():
                        return f1(model(x), y)

                def fused():
                    return model.evaluate(x, y).f1()
            else:
                def literal():
                    with torch.no_grad():
                        return float(accuracy(model(x), y))

                def fused():
                    return float(model.evaluate(x, y).accuracy())

            with step_limit(a.step_limit, f"{case} {name} first calls"):
                va, vb = literal(), fused()  # (and each side's first-call costs)
                literal(), fused()
            ta, tb = [], []
            with step_limit(a.step_limit, f"{case} {name} alternating samples"):
                for _ in range(a.samples):
                    for fn, ts in ((literal, ta), (fused, tb)):
                        torch.cuda.synchronize()
                        t0 = perf_counter()
                        fn()
                        ts.append((perf_counter() - t0) * 1e6)
            ta, tb = np.array(ta), np.array(tb)
            gain = np.median(ta) - np.median(tb)
            sd = max(ta.std(ddof=1), tb.std(ddof=1))
            same = np.allclose(np.atleast_1d(va), np.atleast_1d(vb), rtol=0, atol=1e-12)
            say(f"{case} {M} x {K} x {C} {name}: (a) literal {np.median(ta):8.1f} us (sd {ta.std(ddof=1):.1f}, "
                f"{ta.min():.1f} .. {ta.max():.1f})  (b) evaluate {np.median(tb):8.1f} us (sd "
                f"{tb.std(ddof=1):.1f}, {tb.min():.1f} .. {tb.max():.1f})  a - b {gain:.1f} us = "
                f"{gain / sd:.1f} sd  faster by > 3 sd: {'yes' if gain > 3 * sd else 'NO'}  "
                f"same value: {'yes' if same else f'NO {va} {vb}'}")

            # the forward launch alone
            logits = torch.empty((M, C), dtype=torch.float32, device=dev)
            pred = torch.empty(M, dtype=torch.int64, device=dev)
            stream = _lib.stream_handle(dev)
            if name == "float32":
                ws_bytes = lib.sgc_linear_eval_workspace(M, K, C)
                kname = lib.sgc_linear_eval_kernel_name(M, K, x.stride(0), C, _lib.ptr(x))
                lname = lib.sgc_linear_kernel_name(M, K, x.stride(0), C, _lib.ptr(x))
            else:
                dt = X16_DTYPES[x.dtype]
                ws_bytes = lib.sgc_linear_eval_x16_workspace(M, K, C)
                kname = lib.sgc_linear_eval_x16_kernel_name(M, K, x.stride(0), C, _lib.ptr(x), dt)
                lname = lib.sgc_linear_x16_kernel_name(M, K, x.stride(0), C, _lib.ptr(x), dt)
            if kname == b"none":
                say(f"    forward launch: not covered as it lies in memory (pitch {x.stride(0)}): "
                    f"evaluate copies to an even pitch first; not timed")
                continue
            ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)

            def eval_a():
                if name == "float32":
                    rc = lib.sgc_linear_eval_f32(_lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(b), None,
                                                 M, K, C, _lib.ptr(pred), None, None, None,
                                                 _lib.ptr(ws), ws_bytes, stream)
                else:
                    rc = lib.sgc_linear_eval_x16(_lib.ptr(x), dt, x.stride(0), _lib.ptr(W), _lib.ptr(b),
                                                 None, M, K, C, _lib.ptr(pred), None, None, None,
                                                 _lib.ptr(ws), ws_bytes, stream)
                _lib.check(rc, "linear_eval")

            def lin():  # the raw entry as well: both sides pay one ctypes call per launch
                if name == "float32":
                    rc = lib.sgc_linear_f32(_lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(b),
                                            _lib.ptr(logits), logits.stride(0), M, K, C, stream)
                else:
                    rc = lib.sgc_linear_x16(_lib.ptr(x), dt, x.stride(0), _lib.ptr(W), _lib.ptr(b),
                                            _lib.ptr(logits), logits.stride(0), M, K, C, stream)
                _lib.check(rc, "linear")

            te, tl = [], []
            with step_limit(a.step_limit, f"{case} {name} forward launches"):
                for _ in range(a.rounds):
                    tl.append(_median_ms(lin, a.reps, inner=10) * 1e3)
                    te.append(_median_ms(eval_a, a.reps, inner=10) * 1e3)
            te, tl = np.array(te), np.array(tl)
            spread = tl.max() - tl.min()
            ok = np.median(te) <= np.median(tl) + spread
            say(f"    forward launch alone: evaluation {np.median(te):7.1f} us ({te.min():.1f} .. "
                f"{te.max():.1f})  linear {np.median(tl):7.1f} us ({tl.min():.1f} .. {tl.max():.1f}, "
                f"spread {spread:.1f})  evaluation <= linear + spread: {'yes' if ok else 'NO'}")
            say(f"      {kname.decode()}  |  {lname.decode()}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
