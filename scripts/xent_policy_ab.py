"""A/B of the fused fp32 training loops between two builds of the library, both
loaded into this process:

    python scripts/xent_policy_ab.py --parent variants/parent/libsgc_amd.so
                                     [--rounds 9] [--out profiles/xent_policy/ab.log]

sgc_train_lbfgs_f32 (2 steps of LBFGS(lr=1): every launch of the fused
classifier step behind the stop word) and sgc_train_adam_f32 on its general
schedule (adam_kernel = 1: launches A and B, then the reduce + Adam kernel) at
the raw ABI, at the Reddit-train shape 152,410 x 602 x 41 and the Cora train
shape 140 x 1433 x 7.  Per round one sample of each library, the order swapping
per round: the parameters and optimiser state are put back, then a
device-event pair around one call.  One warm-up round, then `rounds` timed
ones.  The bar is the parent measured in this run: the new median must lie
within the parent's own samples (min .. max).  W, b, the optimiser state, the
loss trace and the status table of the two libraries must be bit-equal.

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
from sgc_amd.propagate import warmup  # noqa: E402

SHAPES = [("reddit_train", 152410, 602, 41, 20), ("cora", 140, 1433, 7, 100)]
LBFGS_STEPS, HISTORY = 2, 100


@contextmanager
def step_limit(seconds, what):
    """End the process (status 124) if the step takes longer than `seconds`."""
    def overrun():
        print(f"xent_policy_ab: step '{what}' passed its {seconds} s limit", flush=True)
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def entries(lib, x, y, W0, b0, adam_epochs, stream):
    """{entry: (reset, call, outputs)} of one library on its own buffers."""
    dev, p = x.device, _lib.ptr
    M, K = x.shape
    C = W0.shape[0]

    def buf(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def ws_of(n):
        return buf(max(1, n), dtype=torch.uint8), n

    # L-BFGS
    W, b = W0.clone(), b0.clone()
    n = C * K + C
    st_bytes = lib.sgc_lbfgs_workspace(n, HISTORY)
    st = buf(st_bytes, dtype=torch.uint8)
    _lib.check(lib.sgc_lbfgs_init(p(st), st_bytes, n, HISTORY, stream), "lbfgs_init")
    torch.cuda.synchronize()
    st0 = st.clone()
    losses, table = buf(LBFGS_STEPS), buf(LBFGS_STEPS * 6, dtype=torch.int64)
    ws_l = ws_of(lib.sgc_train_lbfgs_workspace(M, K, C))

    def reset_l():
        W.copy_(W0), b.copy_(b0), st.copy_(st0)

    def call_l():
        return lib.sgc_train_lbfgs_f32(p(x), x.stride(0), p(W), p(b), p(y), M, K, C, p(st),
                                       LBFGS_STEPS, 1.0, 20, 25, 1e-7, 1e-9, p(losses), p(table),
                                       p(ws_l[0]), ws_l[1], stream)
    # Adam, general schedule
    Wa, ba = W0.clone(), b0.clone()
    mom = [buf(C, K), buf(C, K), buf(C), buf(C)]
    trace = buf(adam_epochs)
    ws_a = ws_of(lib.sgc_train_adam_workspace(M, K, C))

    def reset_a():
        Wa.copy_(W0), ba.copy_(b0)
        for m in mom:
            m.zero_()

    def call_a():
        before = lib.sgc_get_tuning(b"adam_kernel")
        lib.sgc_set_tuning(b"adam_kernel", 1)
        rc = lib.sgc_train_adam_f32(p(x), x.stride(0), p(Wa), p(ba), p(y), M, K, C, p(mom[0]),
                                    p(mom[1]), p(mom[2]), p(mom[3]), 0, adam_epochs, 0.2, 0.9, 0.999,
                                    1e-8, 5e-6, p(trace), p(ws_a[0]), ws_a[1], stream)
        lib.sgc_set_tuning(b"adam_kernel", before)
        return rc
    return {
        f"sgc_train_lbfgs_f32 ({LBFGS_STEPS} steps)": (reset_l, call_l, (W, b, st, losses, table)),
        f"sgc_train_adam_f32 general ({adam_epochs} epochs)": (reset_a, call_a,
                                                                 (Wa, ba, *mom, trace)),
    }


def sample_us(reset, call):
    reset()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = call()
    e.record()
    torch.cuda.synchronize()
    if rc:
        raise RuntimeError(f"code {rc}")
    return s.elapsed_time(e) * 1e3


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
    say(f"fused fp32 training, parent build against this one: 1 warm-up + {a.rounds} rounds, a "
        f"sample = one call between two events (us)")
    stream = _lib.stream_handle(dev)
    for name, M, K, C, adam_epochs in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(M, K, generator=g).to(dev)
        teacher = torch.randn(C, K, generator=g).to(dev) / K ** 0.5
        y = (x @ teacher.t() + 0.5 * torch.randn(M, C, generator=g).to(dev)).argmax(1)
        W0 = (torch.randn(C, K, generator=g) / K ** 0.5).to(dev)
        b0 = (0.1 * torch.randn(C, generator=g)).to(dev)
        sides = {side: entries(lib, x, y, W0, b0, adam_epochs, stream)
                 for side, lib in libs.items()}
        for entry in sides["new"]:
            times = {side: [] for side in sides}
            with step_limit(a.step_limit, f"{entry} {name}"):
                for r in range(1 + a.rounds):
                    for side in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
                        t = sample_us(*sides[side][entry][:2])
                        if r:
                            times[side].append(t)
                same = all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in
                           zip(sides["parent"][entry][2], sides["new"][entry][2]))
            tp, tn = np.array(times["parent"]), np.array(times["new"])
            ok = tp.min() <= np.median(tn) <= tp.max()
            misses += (not ok) + (not same)
            say(f"{entry} {name} {M} x {K} x {C}: parent {np.median(tp):9.1f} us "
                f"({tp.min():.1f} .. {tp.max():.1f})  new {np.median(tn):9.1f} us "
                f"({tn.min():.1f} .. {tn.max():.1f})  new median within the parent's range: "
                f"{'yes' if ok else 'NO'}  outputs bit-equal: {'yes' if same else 'NO'}")
            say("  parent " + " ".join(f"{v:.1f}" for v in tp))
            say("  new    " + " ".join(f"{v:.1f}" for v in tn))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if misses else 0


if __name__ == "__main__":
    sys.exit(main())
