"""One SHA-256 per case over what the two L-BFGS engines compute: the final
parameters, every closure loss and status read on the way, and the whole device
state.  Run on two builds on the same machine, the outputs must be equal line
for line (profiles/lbfgs_shared/bits.txt): a refactor of csrc/lbfgs*.hip or of
sgc_amd/optim.py that changes one bit anywhere changes a hash.

The cases are the smallest shapes that reach each code path: the narrow
kernel's five size classes stepwise on three tensors at odd offsets (history 3:
the ring wraps), its fused calls on fp32 and bf16 features, the wide engine's
three tile cuts stepwise (history 2), a pair it rejects, a NaN loss, and its
fused call with and without a bias.  All inputs are seeded on the CPU.

    python scripts/lbfgs_bits.py [--out FILE]
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def split3(n):
    """Three tensor sizes summing to n, the second and third at odd offsets."""
    a = 13 if n > 40 else 3
    b = ((n - a) // 2) | 1
    return [a, b - a % 2, n - a - (b - a % 2)]


def stepwise(lib, wide, n, hs, kind="quadratic", steps=2, max_iter=5):
    """Raw ABI: `steps` steps of max_iter [closure, iterate] on a seeded
    problem.  quadratic: f = 0.5 sum a (x - c)^2; linear: f = c . x, whose
    gradient never changes, so y = 0 and every pair is rejected (ys <= 1e-10);
    nan: the quadratic with a NaN loss handed in at the fourth closure."""
    from sgc_amd import _lib
    w = "wide_" if wide else ""
    f = lambda name: getattr(lib, f"sgc_lbfgs_{w}{name}")  # noqa: E731
    g = torch.Generator().manual_seed(1000 + n)
    a = (torch.rand(n, generator=g) + 0.5).to(DEV)
    c = torch.randn(n, generator=g).to(DEV)
    x0 = torch.randn(n, generator=g)
    sizes = split3(n)
    assert sum(sizes) == n and all(s > 0 for s in sizes)
    ps = [t.clone().to(DEV) for t in x0.split(sizes)]
    offs = [0, sizes[0], sizes[0] + sizes[1], n]
    nbytes = f("workspace")(n, hs)
    state = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = _lib.stream_handle(DEV)
    _lib.check(f("init")(_lib.ptr(state), nbytes, n, hs, stream), "init")
    nt = len(ps)
    p_ptrs = (ctypes.c_void_p * nt)(*[p.data_ptr() for p in ps])
    numels = (ctypes.c_int64 * nt)(*sizes)
    trace, closures = [], 0
    for _ in range(steps):
        _lib.check(f("begin_step")(_lib.ptr(state), stream), "begin_step")
        for _ in range(max_iter):
            x = torch.cat(ps)
            if kind == "linear":
                grad, loss = c.clone(), (c * x).sum().reshape(1)
            else:
                grad, loss = a * (x - c), (0.5 * (a * (x - c) ** 2).sum()).reshape(1)
            closures += 1
            if kind == "nan" and closures == 4:
                loss = torch.full((1,), float("nan"), device=DEV)
            gs = [grad[offs[i]:offs[i + 1]].contiguous() for i in range(nt)]
            g_ptrs = (ctypes.c_void_p * nt)(*[t.data_ptr() for t in gs])
            _lib.check(f("iterate_f32")(_lib.ptr(state), nt, p_ptrs, g_ptrs, numels, _lib.ptr(loss),
                                        1.0, max_iter, max_iter * 5 // 4, 1e-7, 1e-9, stream),
                       "iterate")
            torch.cuda.synchronize()
            trace.append(loss)
        out = (ctypes.c_int64 * 6)()
        _lib.check(f("read_status")(_lib.ptr(state), out, stream), "read_status")
        trace.append(torch.tensor(list(out), dtype=torch.int64))
    return digest(*ps, *trace, state), tuple(out)


def fused(wide, M, K, C, bias=True, dtype=torch.float32, l2=0.0, steps=2):
    """optim.LBFGS.run_steps on its fused path."""
    from sgc_amd.optim import LBFGS
    if wide:
        from sgc_amd.textsgc import SGC
        model = SGC(K, C, bias=bias).to(DEV)
    else:
        from sgc_amd.models import SGC
        model = SGC(K, C).to(DEV)
    g = torch.Generator().manual_seed(7 * K + C)
    X = (torch.rand(M, K, generator=g) / 4.0).to(DEV).to(dtype)
    y = torch.randint(0, C, (M,), generator=g).to(DEV)
    with torch.no_grad():
        model.W.weight.copy_((torch.randn(C, K, generator=g) * 0.05).to(DEV))
        if model.W.bias is not None:
            model.W.bias.copy_((torch.randn(C, generator=g) * 0.05).to(DEV))
    opt = LBFGS(model.parameters(), max_iter=6, history_size=3, wide=wide)
    losses = opt.run_steps(model, X, y, steps, l2=l2)
    if opt.step_statuses[0] is None or opt._dev_wide != wide:
        raise RuntimeError("the fused call was not taken")
    torch.cuda.synchronize()
    statuses = torch.tensor(opt.step_statuses, dtype=torch.int64)
    return (digest(*[p.data for p in model.parameters()], losses, statuses, opt._dev_state),
            opt.last_status)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sgc_amd import _lib
    lib = _lib.load()
    cases = []
    for n in (70, 4097, 8193, 16385, 65536):  # NV = 1, 2, 4, 8 (streamed rows), 16
        cases.append((f"narrow step n={n} hs=3", lambda n=n: stepwise(lib, False, n, 3)))
    cases.append(("narrow fused f32 37x64x5", lambda: fused(False, 37, 64, 5)))
    cases.append(("narrow fused bf16 37x64x5", lambda: fused(False, 37, 64, 5,
                                                             dtype=torch.bfloat16)))
    for n in (65537, 262145, 1048577):  # tile nv = 1, 2, 4
        cases.append((f"wide step n={n} hs=2", lambda n=n: stepwise(lib, True, n, 2)))
    cases.append(("wide step n=65537 hs=2 rejected pairs",
                  lambda: stepwise(lib, True, 65537, 2, kind="linear")))
    cases.append(("wide step n=65537 hs=2 NaN loss",
                  lambda: stepwise(lib, True, 65537, 2, kind="nan")))
    cases.append(("narrow step n=70 hs=3 NaN loss",
                  lambda: stepwise(lib, False, 70, 3, kind="nan")))
    for bias in (True, False):
        cases.append((f"wide fused 37x2100x33 bias={bias} l2=5e-4",
                      lambda bias=bias: fused(True, 37, 2100, 33, bias=bias, l2=5e-4)))
    lines = []
    for name, fn in cases:
        sha, status = fn()  # status: (n_iter, func_evals, iters, evals, stop, hist_len)
        lines.append(f"{sha}  {name}  last status {tuple(int(v) for v in status)}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
