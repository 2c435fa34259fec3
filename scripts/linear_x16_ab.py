"""A/B of the classifier on float32, bfloat16 and float16 features at the
Reddit-train shape (152,410 x 602, 41 classes), the three types interleaved in
one process:

    python scripts/linear_x16_ab.py [--rounds 5] [--reps 20] [--out profiles/linear_x16/ab.log]

Per round and type: the forward (propagate.linear), the weight backward
(propagate.linear_backward) and the reference closure as written
(zero_grad; F.cross_entropy(model(x), y).backward()).  Event timing as
classifier_bench._median_ms: forward and backward per call over 10
back-to-back calls, the closure per single call; a warm-up for every shape and
type before each sample.  Reports, per type, the median over the rounds, the
rounds' spread (min .. max; the float32 spread is the run's noise floor) and
each time's share of the 8 TB/s bound for the bytes that launch has to move
(X once, plus the logits or dY).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import _lib  # noqa: E402
from sgc_amd.classifier_bench import HBM_PEAK_GBS, _median_ms  # noqa: E402
from sgc_amd.models import SGC  # noqa: E402
from sgc_amd.propagate import X16_DTYPES, linear, linear_backward, warmup  # noqa: E402

TYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=152410)
    ap.add_argument("--features", type=int, default=602)
    ap.add_argument("--classes", type=int, default=41)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M, K, C = a.rows, a.features, a.classes
    dev = torch.device("cuda", 0)
    warmup(dev)
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn(M, K, generator=g).to(dev)
    teacher = torch.randn(C, K, generator=g).to(dev) / K ** 0.5
    y = (x32 @ teacher.t() + 0.5 * torch.randn(M, C, generator=g).to(dev)).argmax(1)
    dY = torch.randn(M, C, generator=g).to(dev)
    torch.manual_seed(0)
    model = SGC(K, C).to(dev)
    W, b = model.W.weight.detach(), model.W.bias.detach()
    xs = {name: x32.to(dt) for name, dt in TYPES}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"classifier A/B, {M} x {K}, {C} classes, {a.rounds} rounds x {a.reps} reps "
        f"(forward / backward: 10 back-to-back calls per sample; closure: single calls)")
    for name, dt in TYPES:
        x = xs[name]
        if dt == torch.float32:
            fk = lib.sgc_linear_kernel_name(M, K, x.stride(0), C, _lib.ptr(x)).decode()
            bk = lib.sgc_linear_backward_kernel_name(M, K, x.stride(0), C, _lib.ptr(x)).decode()
        else:
            fk = lib.sgc_linear_x16_kernel_name(M, K, x.stride(0), C, _lib.ptr(x),
                                                X16_DTYPES[dt]).decode()
            bk = lib.sgc_linear_backward_x16_kernel_name(M, K, x.stride(0), C, _lib.ptr(x),
                                                         X16_DTYPES[dt]).decode()
        say(f"  {name}: forward {fk}; backward {bk}")

    def closure(x):
        def run():
            model.zero_grad(set_to_none=False)
            loss = F.cross_entropy(model(x), y)
            loss.backward()
            return loss
        return run

    res = {name: {"forward": [], "backward": [], "closure": []} for name, _ in TYPES}
    for r in range(a.rounds):
        for name, _ in TYPES:  # interleaved: every round times every type
            x = xs[name]
            res[name]["forward"].append(_median_ms(lambda: linear(x, W, b), a.reps, inner=10))
            res[name]["backward"].append(_median_ms(lambda: linear_backward(x, dY), a.reps, inner=10))
            res[name]["closure"].append(_median_ms(closure(x), a.reps))
        say(f"round {r}: " + "  ".join(
            f"{name} fwd {res[name]['forward'][-1] * 1e3:.1f} bwd {res[name]['backward'][-1] * 1e3:.1f} "
            f"closure {res[name]['closure'][-1] * 1e3:.1f} us" for name, _ in TYPES))
    say("medians over the rounds (min .. max), share of the 8 TB/s bound:")
    for name, dt in TYPES:
        es = 4 if dt == torch.float32 else 2
        nbytes = {"forward": es * M * K + 4 * M * C + 4 * C * K, "backward": es * M * K + 4 * M * C}
        for what in ("forward", "backward", "closure"):
            v = np.array(res[name][what]) * 1e3
            tail = ""
            if what in nbytes:
                bound = nbytes[what] / HBM_PEAK_GBS / 1e3  # us
                tail = (f"  {nbytes[what] / 1e6:.0f} MB, bound {bound:.1f} us, "
                        f"share {bound / np.median(v):.2f}")
            say(f"  {name:9s} {what:8s} {np.median(v):7.1f} us ({v.min():.1f} .. {v.max():.1f}){tail}")
    f32 = res["float32"]
    for what in ("forward", "backward", "closure"):
        v = np.array(f32[what]) * 1e3
        say(f"  float32 {what} spread across rounds: {v.max() - v.min():.1f} us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
