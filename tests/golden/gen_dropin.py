"""Golden outputs for tests/test_dropin.py, made by RUNNING THE REFERENCE'S OWN
MODULES (normalization, utils, metrics, args) on CPU.

    python tests/golden/gen_dropin.py          # in the build container

The inputs are the seeded ones tests/test_dropin.py builds (its own helpers
are imported from there, so there is one definition of each); inputs whose
generator is not pinned by a stream-compatibility promise (scipy's
sp.random, torch.randn) are stored beside the outputs.  Nothing of the
reference is written to the repo: only what its functions returned.

Output: tests/golden/dropin_reference.npz (arrays) and
tests/golden/dropin_reference.json (argparse namespaces and flags).
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = os.environ.get("SGC_REFERENCE", "/root/reference")


def reference_modules():
    """The reference's modules under their own names (its utils does
    `from normalization import ...`), removed from sys.modules afterwards."""
    mods = {}
    sys.path.insert(0, REF)
    saved = {k: sys.modules.get(k) for k in ("normalization", "utils", "metrics", "args")}
    try:
        for name in ("normalization", "utils", "metrics", "args"):
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, f"{name}.py"))
            m = importlib.util.module_from_spec(spec)
            sys.modules[name] = m
            spec.loader.exec_module(m)
            mods[name] = m
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods


def main():
    sys.path.insert(0, os.path.dirname(TESTS))
    sys.path.insert(0, TESTS)
    import test_dropin as t
    ref = reference_modules()
    arrays, meta = {}, {}

    for kind in t.ADJ_KINDS:
        want = ref["normalization"].aug_normalized_adjacency(t._adj_case(kind))
        arrays[f"augnorm/{kind}/row"] = want.row
        arrays[f"augnorm/{kind}/col"] = want.col
        arrays[f"augnorm/{kind}/data"] = want.data
        meta[f"augnorm/{kind}/format"] = want.getformat()

    X = sp.random(50, 30, density=0.2, random_state=3, format="lil")
    X[3, :] = 0
    arrays["row_normalize/X"] = X.toarray()
    arrays["row_normalize/out"] = ref["normalization"].row_normalize(X).toarray()
    try:
        ref["normalization"].fetch_normalization("NormLap")(sp.eye(3))
        meta["fetch_NormLap_call_raises"] = None
    except Exception as e:  # what the reference does with an unknown name
        meta["fetch_NormLap_call_raises"] = type(e).__name__

    b = ref["utils"].sparse_mx_to_torch_sparse_tensor(t._to_torch_case())
    arrays["to_torch/indices"] = b._indices().numpy()
    arrays["to_torch/values"] = b._values().numpy()
    meta["to_torch"] = {"shape": list(b.shape), "dtype": str(b.dtype),
                        "is_coalesced": bool(b.is_coalesced())}

    cwd = os.getcwd()
    for name in t.CITATION_NAMES:
        with tempfile.TemporaryDirectory() as td:
            t._write_citation_case(td, name)
            os.chdir(td)
            try:
                got = ref["utils"].load_citation(name, "AugNormAdj", cuda=False)
            finally:
                os.chdir(cwd)
        arrays[f"citation/{name}/adj_indices"] = got[0]._indices().numpy()
        arrays[f"citation/{name}/adj_values"] = got[0]._values().numpy()
        meta[f"citation/{name}/adj_shape"] = list(got[0].shape)
        for key, v in zip(t.CITATION_FIELDS, got[1:]):
            arrays[f"citation/{name}/{key}"] = v.numpy()
        assert len(got) == 1 + len(t.CITATION_FIELDS)

    meta["args"] = []
    saved_argv = sys.argv
    for argv in t.ARGV_CASES:
        sys.argv = list(argv)
        try:
            ns = vars(ref["args"].get_citation_args())
        finally:
            sys.argv = saved_argv
        # args.py:39: cuda = not no_cuda and torch.cuda.is_available() -- a
        # property of the host, not stored; the test applies the same rule
        ns.pop("cuda")
        meta["args"].append({"argv": list(argv), "namespace": ns})

    g = torch.Generator().manual_seed(0)
    out = torch.randn(200, 7, generator=g)
    lab = torch.randint(0, 7, (200,), generator=g)
    arrays["metrics/out"] = out.numpy()
    arrays["metrics/lab"] = lab.numpy()
    arrays["metrics/accuracy"] = ref["metrics"].accuracy(out, lab).numpy()
    arrays["metrics/f1"] = np.asarray(ref["metrics"].f1(out, lab), dtype=np.float64)

    np.savez_compressed(os.path.join(HERE, "dropin_reference.npz"), **arrays)
    with open(os.path.join(HERE, "dropin_reference.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items()})


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
