"""A/B of the 16-bit classifier launches between two builds of the library, both
loaded into this process:

    python scripts/x16_stream_ab.py --parent variants/parent/libsgc_amd.so
                                    [--rounds 9] [--out profiles/x16_stream/ab.log]

The entries at the raw ABI with preallocated buffers, at the shapes the project
reports: sgc_linear_x16, sgc_linear_backward_x16 and sgc_linear_xent_x16 at
152,410 x 602 x 41, sgc_linear_eval_x16 (predictions only) at 55,334 x 602 x 41,
bfloat16 and float16.  Per round one sample of each library, parent first: a
device-event pair around 20 back-to-back calls, the time per call.  One warm-up
round, then `rounds` timed ones.  The bar is the parent measured in this run:
the new median may exceed the parent's by no more than the parent's own spread
(max - min over its rounds).  Every output of the two libraries on the timed
operands must be bit-equal.

Every step runs under its own time limit: a step that overruns ends the
process with status 124.
"""
import argparse
import os
import sys
import threading
from contextlib import contextmanager

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgc_amd import _lib  # noqa: E402
from sgc_amd.propagate import X16_DTYPES, warmup  # noqa: E402

CALLS = 20


@contextmanager
def step_limit(seconds, what):
    """End the process (status 124) if the step takes longer than `seconds`."""
    def overrun():
        print(f"x16_stream_ab: step '{what}' passed its {seconds} s limit", flush=True)
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def entries(lib, x, W, b, y, dY, stream):
    """{entry: (call, outputs)} of one library on its own output buffers."""
    dev = x.device
    M, K = x.shape
    C = W.shape[0]
    dt, ldx, p = X16_DTYPES[x.dtype], x.stride(0), _lib.ptr

    def buf(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def ws_of(n):
        return buf(max(1, n), dtype=torch.uint8), n

    Y = buf(M, C)
    dW, db, ws_b = buf(C, K), buf(C), ws_of(lib.sgc_linear_backward_x16_workspace(M, K, C))
    loss, gW, gb, ws_x = buf(1), buf(C, K), buf(C), ws_of(lib.sgc_linear_xent_x16_workspace(M, K, C))
    Me = 55334
    pred, ws_e = buf(Me, dtype=torch.int64), ws_of(lib.sgc_linear_eval_x16_workspace(Me, K, C))
    return {
        "sgc_linear_x16": (lambda: lib.sgc_linear_x16(
            p(x), dt, ldx, p(W), p(b), p(Y), Y.stride(0), M, K, C, stream), (Y,)),
        "sgc_linear_backward_x16": (lambda: lib.sgc_linear_backward_x16(
            p(x), dt, ldx, p(dY), dY.stride(0), M, K, C, p(dW), p(db), p(ws_b[0]), ws_b[1], stream),
            (dW, db)),
        "sgc_linear_xent_x16": (lambda: lib.sgc_linear_xent_x16(
            p(x), dt, ldx, p(W), p(b), p(y), M, K, C, p(loss), p(gW), p(gb), p(ws_x[0]), ws_x[1],
            stream), (loss, gW, gb)),
        "sgc_linear_eval_x16 (pred only)": (lambda: lib.sgc_linear_eval_x16(
            p(x), dt, ldx, p(W), p(b), None, Me, K, C, p(pred), None, None, None, p(ws_e[0]),
            ws_e[1], stream), (pred,)),
    }


def sample_us(call):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(CALLS):
        rc = call()
    e.record()
    torch.cuda.synchronize()
    if rc:
        raise RuntimeError(f"code {rc}")
    return s.elapsed_time(e) / CALLS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-limit", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    libs = {"parent": _lib.load_path(os.path.abspath(a.parent)), "new": _lib.load()}
    lines, misses = [], 0

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with step_limit(a.step_limit, "warm-up"):
        warmup(dev)
    say(f"x16 launches, parent build against this one: 1 warm-up + {a.rounds} rounds, a sample = "
        f"{CALLS} back-to-back calls between two events (us per call)")
    M, K, C = 152410, 602, 41
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn(M, K, generator=g)
    W = (torch.randn(C, K, generator=g) / K ** 0.5).to(dev)
    b = (0.1 * torch.randn(C, generator=g)).to(dev)
    y = torch.randint(0, C, (M,), generator=g).to(dev)
    dY = (torch.randn(M, C, generator=g) / M).to(dev)
    stream = _lib.stream_handle(dev)
    for name, dtype in (("bfloat16", torch.bfloat16), ("float16", torch.float16)):
        x = x32.to(dtype).to(dev)
        sides = {side: entries(lib, x, W, b, y, dY, stream) for side, lib in libs.items()}
        for entry in sides["new"]:
            times = {side: [] for side in sides}
            with step_limit(a.step_limit, f"{entry} {name}"):
                for r in range(1 + a.rounds):
                    for side in ("parent", "new"):
                        t = sample_us(sides[side][entry][0])
                        if r:
                            times[side].append(t)
                same = all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in
                           zip(sides["parent"][entry][1], sides["new"][entry][1]))
            tp, tn = np.array(times["parent"]), np.array(times["new"])
            spread = tp.max() - tp.min()
            ok = np.median(tn) <= np.median(tp) + spread
            misses += (not ok) + (not same)
            say(f"{entry} {name}: parent {np.median(tp):7.1f} us ({tp.min():.1f} .. {tp.max():.1f}, "
                f"spread {spread:.1f})  new {np.median(tn):7.1f} us ({tn.min():.1f} .. {tn.max():.1f})  "
                f"new <= parent + spread: {'yes' if ok else 'NO'}  outputs bit-equal: "
                f"{'yes' if same else 'NO'}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if misses else 0


if __name__ == "__main__":
    sys.exit(main())
