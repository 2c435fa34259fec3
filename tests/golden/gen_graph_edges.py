"""Golden outputs for the graph-construction edge cases, made by RUNNING THE
REFERENCE'S OWN MODULES (normalization, utils) on CPU.

    python tests/golden/gen_graph_edges.py          # in the build container

For every case of tests/graph_edge_cases.py:
    sparse_mx_to_torch_sparse_tensor(aug_normalized_adjacency(A)).float()
and, for the slice-then-normalise case, the same of A[idx, :][:, idx].  The
inputs are stored beside the outputs (numpy's Generator streams are not
promised stable).  Nothing of the reference is written to the repo: only what
its functions returned.

Output: tests/golden/graph_edges.npz
    <case>/indptr, indices, data      the input A (canonical CSR, fp64)
    <case>/row, col, val              the reference's S (COO order, fp32)
    sub/idx, sub/row, sub/col, sub/val   the sliced case
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def reference_s(ref, A):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # power/multiply on NaN and inf, FloatTensor ctor
        with np.errstate(all="ignore"):
            t = ref["utils"].sparse_mx_to_torch_sparse_tensor(
                ref["normalization"].aug_normalized_adjacency(A)).float()
    idx = t._indices().numpy()
    return idx[0].astype(np.int64), idx[1].astype(np.int64), t._values().numpy().astype(np.float32)


def main():
    sys.path.insert(0, os.path.dirname(TESTS))
    sys.path.insert(0, TESTS)
    sys.path.insert(0, HERE)
    import graph_edge_cases as g
    from gen_dropin import reference_modules
    ref = reference_modules()
    arrays = {}
    for name, A in g.cases().items():
        arrays[f"{name}/indptr"] = A.indptr.astype(np.int32)
        arrays[f"{name}/indices"] = A.indices.astype(np.int32)
        arrays[f"{name}/data"] = A.data.astype(np.float64)
        row, col, val = reference_s(ref, A)
        arrays[f"{name}/row"], arrays[f"{name}/col"], arrays[f"{name}/val"] = row, col, val
    A = g.cases()[g.SUBGRAPH_CASE]
    idx = g.subgraph_index(A.shape[0])
    arrays["sub/idx"] = idx
    arrays["sub/row"], arrays["sub/col"], arrays["sub/val"] = reference_s(ref, A[idx, :][:, idx])
    out = os.path.join(HERE, "graph_edges.npz")
    with open(out, "wb") as f:      # fixed member order and timestamps: byte-identical reruns
        import zipfile
        with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as z:
            for key in sorted(arrays):
                info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                with z.open(info, "w") as m:
                    np.lib.format.write_array(m, np.ascontiguousarray(arrays[key]),
                                              allow_pickle=False)
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items() if "/row" in k})


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
