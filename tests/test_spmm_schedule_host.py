"""The SpMM's schedule choice (sgc_amd/csrc/spmm_schedule.h), checked without a GPU.

1. spmm_schedule_host.cpp, compiled against the header with the host C++
   compiler (and once more with -fsanitize=address,undefined where the compiler
   links it), asserts the whole SpmmSchedule of the benchmark shapes and of
   every (F, layout, knob) combination the GPU suites' docstrings name, against
   literals taken from launch_spmm as it stood before the header existed.
2. sgc_spmm_kernel_name (host only: no device) for the parametrisations of
   tests/test_gpu_ieee_operands.py's test_one_hop_every_schedule,
   test_heavy_row_bodies and test_hub_kernel_knobs: the kernel body each
   docstring claims is the one the library would launch, and the test file's
   own v4_ok agrees with the schedule.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ieee_operands as io
import test_gpu_ieee_operands as suite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = suite.N
X_PADDED, Y_PADDED, HUB_SERIAL, LIGHT_ORDER, X_UNDER_4G = 1, 2, 32, 64, 128
BASE = 0x7F0000000000  # an address as aligned as an allocation's; never dereferenced


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


@pytest.mark.parametrize("sanitize", [False, True])
def test_schedule_literals(tmp_path, sanitize):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "spmm_schedule_host")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sgc_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"),
           os.path.join(ROOT, "tests", "spmm_schedule_host.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        if subprocess.run(cmd, capture_output=True).returncode != 0:
            pytest.skip("the host compiler does not link the sanitizer runtimes")
    else:
        subprocess.run(cmd, check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert " 0 failures" in res.stdout
    assert int(res.stdout.split(" cases")[0].split()[-1]) >= 450


# ---- sgc_spmm_kernel_name ----------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from sgc_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def degrees():
    return np.diff(io.edge_graph(N, 0, "wild").row_ptr)


def _plan(deg, th, hub, ts):
    """What DeviceCSR.plan() and wide_args() give spmm() for (th, hub): the counts
    of the sorted plan and its launch flags, restated from the degrees."""
    hub = max(hub, th)
    n_heavy, n_hub = int((deg > th).sum()), int((deg > hub).sum())
    flags = (HUB_SERIAL if n_hub and deg.max() <= 3072 else 0) | (LIGHT_ORDER if N > n_heavy else 0)
    wide = (max(0, int((deg > ts).sum()) - n_heavy), ts) if ts > 0 and N > n_heavy else (-1, 0)
    return n_heavy, n_hub, flags, int((deg > 0).sum()), wide


Knobs = suite.knobs  # sets and restores through sgc_set_tuning: no device is touched


SCHED = re.compile(r"^(spmm_rows_kernel|spmm_csr_kernel)<([^>]*)> LR=(\d+) slices=(\d+) n_sub=(\d+) "
                   r"bits=(\d+) grid=(\d+)x(\d+) wide=(\d+) hub=(\w+)(?: spmm_hub_kernel<(\d+),(\d+)> "
                   r"grid=(\d+))?$")


def schedule(lib, deg, F, how, th, hub):
    """The parsed sgc_spmm_kernel_name of the launch suite._one_hop makes."""
    lay = suite.Layout(how, F)  # geometry and flags only: nothing is allocated
    ts = int(lib.sgc_get_tuning(b"short_wide_ts"))
    n_heavy, n_hub, pflags, n_nonempty, wide = _plan(deg, th, hub, ts)
    u4g = X_UNDER_4G if N * lay.ld * 4 < (1 << 32) else 0
    name = lib.sgc_spmm_kernel_name(0, N, BASE + 4 * lay.off, lay.ld, BASE + (1 << 30) + 4 * lay.off,
                                    lay.ld, F, BASE + (1 << 31), n_heavy, n_hub, th,
                                    lay.flags | pflags | u4g, n_nonempty, wide[0], wide[1]).decode()
    m = SCHED.match(name)
    assert m, name
    t = dict(kv.split("=") for kv in m.group(2).split(","))
    return dict(kernel=m.group(1), name=name, LR=int(m.group(3)), slices=int(m.group(4)),
                n_sub=int(m.group(5)), bits=int(m.group(6)), wide=int(m.group(9)), hub=m.group(10),
                hub_kernel=(int(m.group(11)), int(m.group(12))) if m.group(11) else None,
                **{k: int(v) for k, v in t.items()})


@pytest.mark.parametrize("F,how", [(F, how) for F in suite.WIDTHS
                                   for how in ("lines", "contig", "slice")])
def test_v4_ok_agrees_with_the_schedule(lib, degrees, F, how):
    """rows_per_wave = 2 takes the multi-row kernel exactly where 16-B lanes are
    possible: the suite's v4_ok restates launch_spmm's."""
    with Knobs(rows_per_wave=2):
        s = schedule(lib, degrees, F, how, 40, 500)
    assert (s["kernel"] == "spmm_rows_kernel") == suite.v4_ok(F, how), s["name"]


@pytest.mark.parametrize("F,how,rows_per_wave", suite.ONE_HOP)
def test_one_hop_bodies(lib, degrees, F, how, rows_per_wave):
    """The bodies test_one_hop_every_schedule's docstring names."""
    for th, hub in [(0, 0), (0, 10**9), (16, 200), (40, 500), (10**9, 10**9)]:
        with Knobs(rows_per_wave=rows_per_wave):
            s = schedule(lib, degrees, F, how, th, hub)
        F4 = (F + 3) // 4 * 4
        if not suite.v4_ok(F, how):
            # row_chunks_pipe with 1- or 2-float lanes (4-float lanes only where F4 < 32
            # alone rules the multi-row kernel out: 12 floats in 16-B aligned rows)
            assert s["kernel"] == "spmm_csr_kernel", s["name"]
            assert s["V"] <= 2 or (F4 < 32 and how != "slice" and F % 4 == 0), s["name"]
        elif rows_per_wave in (2, 4) or (rows_per_wave == 0 and F4 < 128):
            assert s["kernel"] == "spmm_rows_kernel", s["name"]
            assert 9 <= s["LR"] <= 32 and s["slices"] == -(-F4 // (4 * s["LR"])), s["name"]
            if F4 >= 128:
                assert s["LR"] == (16 if rows_per_wave == 4 else 32), s["name"]
            # 1..5 slices; only 602 floats at the forced 16 lanes per row takes 10
            assert s["slices"] <= 5 or (F == 602 and rows_per_wave == 4 and s["slices"] == 10)
        elif rows_per_wave == 1:
            # 16-B lanes where the computed width is a multiple of 4 (F itself, or F
            # rounded up in padded rows at 129..256 floats), else 1- or 2-float lanes
            assert s["kernel"] == "spmm_csr_kernel", s["name"]
            assert (s["V"] == 4) == (F % 4 == 0 or 128 < F4 <= 256), s["name"]
        elif F in (130, 152, 256):  # rows_per_wave 0: the one-row kernel with 16-B lanes
            assert s["kernel"] == "spmm_csr_kernel" and s["V"] == 4 and s["slices"] == 1, s["name"]
        else:  # 602 in 128-B rows: the small-wide rule's 512-float slices
            assert F == 602 and s["kernel"] == "spmm_csr_kernel", s["name"]
            assert s["V"] * s["C"] * 64 == 512, s["name"]
        # hub rows: every hub here is serial (3001 <= 3072 nonzeros) -- fused into the
        # light launch or spmm_hub_kernel before it, never beside it
        n_hub = int((degrees > max(hub, th)).sum())
        assert (s["hub"] in ("fused", "serial")) == (n_hub > 0), s["name"]
        assert (s["hub"] == "none") == (n_hub == 0), s["name"]


HEAVY_CASES = [(30, "lines", 0), (32, "contig", 0), (33, "lines", 0), (64, "contig", 0),
               (65, "lines", 0), (130, "lines", 2), (602, "lines", 2), (152, "contig", 1),
               (256, "lines", 0), (3, "slice", 0)]


@pytest.mark.parametrize("heavy_pairs", [0, 1, 5, 13, 17, 29, 31])
@pytest.mark.parametrize("F,how,rows_per_wave", HEAVY_CASES)
def test_heavy_row_bodies(lib, degrees, F, how, rows_per_wave, heavy_pairs):
    """The bodies test_heavy_row_bodies' docstring names, per heavy_pairs bit."""
    for th, hub in [(0, 10**9), (16, 200), (40, 500)]:
        with Knobs(rows_per_wave=rows_per_wave, heavy_pairs=heavy_pairs):
            s = schedule(lib, degrees, F, how, th, hub)
        if F in (30, 32):    # bit 4: row_quads_pipe at 32 computed floats
            assert s["kernel"] == "spmm_rows_kernel" and s["QV"] == (2 if heavy_pairs & 4 else 0)
        elif F in (33, 64):  # bit 8: row_quadsT_pipe, without it the pairs / sub-chunks
            assert s["kernel"] == "spmm_rows_kernel" and s["QV"] == (4 if heavy_pairs & 8 else 0)
        elif F in (65, 130, 602):  # bit 1 pairs (one item per row and slice), bit 16 transposed
            assert s["kernel"] == "spmm_rows_kernel" and s["QV"] == 0, s["name"]
            assert s["bits"] == heavy_pairs & 17, s["name"]
            sub = 64 * s["VH"]  # without bit 1: row_chunks_pipe items of 64 * VH floats
            assert s["n_sub"] == (1 if heavy_pairs & 1 else
                                  (min((F + 3) // 4 * 4, 128) + sub - 1) // sub), s["name"]
        elif F in (152, 256):  # bit 2: row_pairs_pipe inside spmm_csr_kernel's 16-B-lane items
            assert s["kernel"] == "spmm_csr_kernel" and s["V"] == 4, s["name"]
            assert s["bits"] == (heavy_pairs >> 1) & 1, s["name"]
        else:  # 3 floats: 4-B lanes, no bit applies to the lanes
            assert s["kernel"] == "spmm_csr_kernel" and s["V"] == 1, s["name"]
        if s["kernel"] == "spmm_rows_kernel" and s["QV"]:
            assert s["n_sub"] == 1 and s["VH"] == 2 and s["LR"] <= 16, s["name"]


@pytest.mark.parametrize("hub_chunk", [0, 32, 64])
@pytest.mark.parametrize("F,how", [(64, "lines"), (130, "lines"), (152, "lines"), (65, "slice"),
                                   (602, "lines")])
def test_hub_kernel_knobs(lib, degrees, F, how, hub_chunk):
    """The hub launches test_hub_kernel_knobs' docstring names."""
    for loaders in (15, 7):
        for stream in (0, 1, 2):
            for fuse in (0, 1):
                for th, hub in [(0, 0), (16, 200), (40, 500)]:
                    with Knobs(hub_chunk=hub_chunk, hub_loaders=loaders, hub_stream=stream,
                               hub_fuse=fuse):
                        s = schedule(lib, degrees, F, how, th, hub)
                    what = (s["name"], loaders, stream, fuse)
                    can_fuse = hub_chunk == 0 and fuse == 1 and stream != 1
                    if s["hub"] == "fused":
                        assert can_fuse and "HF=32" in s["name"], what
                        continue
                    # the launches that can take fused items: the one-row kernel's
                    # single 16-B-lane chunk (130 / 152 floats in padded 128-B rows)
                    assert not (can_fuse and F in (130, 152)), what
                    assert s["hub"] == ("concurrent" if stream == 1 else "serial"), what
                    chunk = hub_chunk or (32 if how == "lines" and F <= 192 else 64)
                    assert s["hub_kernel"] == (chunk, loaders), what


def test_name_of_nothing_to_launch(lib):
    assert lib.sgc_spmm_kernel_name(0, 0, BASE, 64, BASE, 64, 64, None, 0, 0, 0, 0, -1, -1,
                                    0) == b"none"
    assert lib.sgc_spmm_kernel_name(0, 8, BASE, 64, BASE, 64, 64, None, 0, 0, 0, 1 << 20, -1, -1,
                                    0) == b"none"
    assert b"unknown flags" in lib.sgc_last_error()
