"""The four sgc_spmm_csr_f32* generations and the three launch-list recorders
fill one call struct (csrc/internal.h: SpmmCall): each narrower generation
must write the bytes sgc_spmm_csr_f32_ex3 writes with the neutral arguments
(-1, -1, 0) in the places it lacks, and a list recorded through each recorder
the bytes of the direct launch.  sgc_spmm_csr_f32_ex3 with the plan's real
counts is compared with the oracle, as tests/test_gpu_short_wide.py and the
IEEE suite do (ieee_operands.compare's rule).

Operands: the IEEE suite's graph (N = 4096) at 130 and 602 floats in 128-B
rows, the sorted plan, short_wide = 16 forced -- with rows_per_wave = 2 and
hub_fuse = 0, where the launch takes wide items (the counter is asserted).
"""
import ctypes

import pytest
import torch

import ieee_operands as io
import test_gpu_ieee_operands as suite

pytestmark = pytest.mark.gpu

N = suite.N
TS = 16


def _bytes_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("F", [130, 602])
def test_every_generation_and_recorder_writes_the_same_bytes(F):
    from sgc_amd import _lib
    from sgc_amd.propagate import SLOT_FIXED, spmm_args, wide_args, x_flags
    lib = _lib.load()
    csr = suite.device_csr()
    want, want_dev = suite.reference("wild", F)
    lay = suite.Layout("lines", F)
    X = lay.x(io.edge_features(N, F, "wild"))
    stream = _lib.stream_handle(X.device)

    with suite.knobs(short_wide=TS, rows_per_wave=2, hub_fuse=0):
        pl = csr.plan(0, N, None, None, F)
        assert pl.ordered and pl.n_nonempty >= 0 and len(pl.above) == 4, "not the sorted plan"
        flags = lay.flags | pl.hub_flags() | x_flags(X)
        wide = wide_args(csr, pl, 0, N)
        assert wide[1] == TS and wide[0] >= 0

        def direct(fn, flags, tail, plain=False):
            """One launch through generation `fn`: spmm_args up to the threshold, then
            (flags unless `plain`) + tail + stream; returns the whole NaN-prefilled buffer."""
            buf, out = lay.out(N)
            a = spmm_args(csr, pl, 0, N, X, out, flags, ())
            head = a[:14] if plain else a[:15]  # ..., threshold[, flags] (n_nonempty dropped)
            _lib.check(fn(*head, *tail, stream), "spmm")
            return buf

        def recorded(fn, flags, tail):
            buf, out = lay.out(N)
            a = spmm_args(csr, pl, 0, N, X, out, flags, ())
            h = ctypes.c_int64(0)
            _lib.check(lib.sgc_launch_list_create(ctypes.byref(h)), "launch_list_create")
            try:
                _lib.check(fn(h.value, *a[:15], *tail, SLOT_FIXED, SLOT_FIXED), "launch_list_add")
                _lib.check(lib.sgc_launch_list_run(h.value, None, None, stream), "launch_list_run")
                torch.cuda.synchronize()
            finally:
                lib.sgc_launch_list_destroy(h.value)
            return buf

        ex3 = lib.sgc_spmm_csr_f32_ex3
        before = int(lib.sgc_get_tuning(b"short_wide_launches"))
        full = direct(ex3, flags, (pl.n_nonempty, *wide))
        assert int(lib.sgc_get_tuning(b"short_wide_launches")) == before + 1, "no wide items taken"
        suite.check(full[:, :F], want, want_dev, (F, "ex3, real counts"))
        assert lay.padding_untouched(full)

        # each narrower generation against _ex3 with the neutral arguments
        assert _bytes_equal(direct(lib.sgc_spmm_csr_f32, 0, (), plain=True),
                            direct(ex3, 0, (-1, -1, 0))), "sgc_spmm_csr_f32"
        ex3_no_counts = direct(ex3, flags, (-1, -1, 0))
        assert _bytes_equal(direct(lib.sgc_spmm_csr_f32_ex, flags, ()), ex3_no_counts), "_ex"
        ex3_nonempty = direct(ex3, flags, (pl.n_nonempty, -1, 0))
        assert _bytes_equal(direct(lib.sgc_spmm_csr_f32_ex2, flags, (pl.n_nonempty,)),
                            ex3_nonempty), "_ex2"
        # every schedule of the same launch computes the same chains
        for other in (ex3_no_counts, ex3_nonempty):
            assert _bytes_equal(other, full)

        # a list recorded through each recorder against the direct launch
        assert _bytes_equal(recorded(lib.sgc_launch_list_add_spmm, flags, ()), ex3_no_counts)
        assert _bytes_equal(recorded(lib.sgc_launch_list_add_spmm_ex2, flags, (pl.n_nonempty,)),
                            ex3_nonempty)
        before = int(lib.sgc_get_tuning(b"short_wide_launches"))
        assert _bytes_equal(recorded(lib.sgc_launch_list_add_spmm_ex3, flags,
                                     (pl.n_nonempty, *wide)), full)
        assert int(lib.sgc_get_tuning(b"short_wide_launches")) == before + 1
