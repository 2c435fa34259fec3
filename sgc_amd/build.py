"""Build libsgc_amd.so (gfx950) in-tree with hipcc.

The shared library is the product's native core: HIP kernels for gfx950 plus
the C ABI in include/sgc_amd.h.  It is built in-tree so it travels with the
repo snapshot to the GPU box (see .gitignore: *.so stays out of history).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsgc_amd.so")
SOURCES = ["capi.hip", "spmm.hip", "ingest.hip", "linear.hip", "normalize.hip", "xent.hip",
           "subgraph.hip", "cpu.hip", "mgpu.hip", "plan.hip", "groups.hip", "sort.hip",
           "exchange.hip", "loss.hip", "spmm16.hip", "lbfgs.hip", "linear16.hip", "adam.hip",
           "xent_fwd_stop.hip", "xent16.hip", "eval.hip", "eval16.hip",
           "lbfgs_wide.hip"]


def _headers():
    """Every header a source may include (csrc/*.h and the public ABI)."""
    import glob
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(ROOT, "include",
                                                                        "sgc_amd.h")]
ARCH = os.environ.get("SGC_OFFLOAD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FLAGS = [
    f"--offload-arch={ARCH}",
    "-O3",
    "-std=c++17",
    "-fPIC",
    # IEEE fp32: no FTZ, no contraction beyond the explicit fmaf chains
    "-fno-gpu-flush-denormals-to-zero",
    "-ffp-contract=off",
    "-fno-fast-math",
    "-Wall",
    "-Wno-unused-function",
]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + _headers()
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, out=None, defines=()):
    """Compile the library; `out`/`defines` build tuning variants elsewhere."""
    lib = out or LIB
    if not force and out is None and not _stale():
        return LIB
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    tmp = lib + ".tmp"
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    common = [HIPCC, *FLAGS, *[f"-D{d}" for d in defines], "-I", os.path.join(ROOT, "include"),
              "-I", CSRC]
    # one hipcc per source, in parallel (each source launches only its own
    # kernels, so no relocatable device code is needed), then one link
    # objects in a fixed per-(output, defines) directory: the object paths
    # end up in the code-object bundle, so a fixed path keeps the library
    # byte-identical across rebuilds of the same sources (bench.py ties PMC
    # traffic records to the library's sha256)
    tag = hashlib.sha256(repr((os.path.abspath(lib), tuple(defines))).encode()).hexdigest()[:16]
    td = os.path.join(ROOT, "build", f"obj_{tag}")  # git- and gpurun-ignored
    os.makedirs(td, exist_ok=True)
    objs = [os.path.join(td, os.path.basename(s) + ".o") for s in srcs]
    cmds = [[*common, "-c", s, "-o", o] for s, o in zip(srcs, objs)]
    if verbose:
        print("[sgc_amd] " + " ".join(cmds[0][:-4]) + " -c <source> (x%d, parallel)"
              % len(cmds), file=sys.stderr)
    jobs = max(1, min(len(cmds), int(os.environ.get("MAX_JOBS", os.cpu_count() or 1))))
    with ThreadPoolExecutor(jobs) as ex:
        for f in [ex.submit(subprocess.check_call, c) for c in cmds]:
            f.result()
    subprocess.check_call([HIPCC, *FLAGS, "-shared", *objs, "-o", tmp])
    os.replace(tmp, lib)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv)
