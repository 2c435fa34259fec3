"""One-off: a Python port of the launch_spmm / launch_rows / launch_rows_wide / launch_vc
decisions as they stood in sgc_amd/csrc/spmm.hip at commit 4ee6fe1 (before
spmm_schedule.h), used once to derive the literals of tests/spmm_schedule_cases.inc.
It shares no code with spmm_schedule.h; the Reddit-shape case was also worked by hand."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

XP, YP, NOHUB, HUBONLY, ACC, SERIAL, ORDER, U4G = 1, 2, 4, 8, 16, 32, 64, 128
INT32_MAX = 2**31 - 1
DEF = dict(slice_floats=128, max_vec=4, rows_per_wave=0, heavy_pairs=29, hub_chunk=0, hub_stream=0,
           hub_loaders=15, hub_fuse=1, short_wide=-1, short_wide_first=0)
KN = list(DEF)


def pick_vec(k, F, ldx, ldy, xa, ya):
    for V in (4, 2):
        if V <= k["max_vec"] and F % V == 0 and ldx % V == 0 and ldy % V == 0 and xa % (4 * V) == 0 \
                and ya % (4 * V) == 0:
            return V
    return 1


def parent(n_rows, F, ldx, ldy, xa, ya, flags, has_plan, n_heavy, n_hub, th, n_nonempty, n_not_wide,
           wmax, k):
    E = dict(kernel=-1, multi_row=0, V=0, C=0, LB=0, VH=0, QV=0, HF=0, WD=0, O32=0, LR=0, F_load=0,
             vec_store=0, slices=0, n_sub=0, n_heavy=0, n_light_items=0, n_wide=0, wide_first=0,
             slice_blocks=0, wide_blocks=0, grid_x=0, grid_y=1, kernel_bits=0, hub=0, hub_chunk=0,
             hub_loaders=0, hub_n_chunks=0, hub_grid=0, fused_chunks=0, fused_blocks=0)
    light_rows = False
    n_light = 0
    if (flags & ORDER) and has_plan:
        assert n_heavy <= n_rows
        light_rows = True
        n_light = n_rows - n_heavy
    if light_rows and (flags & ACC) and n_nonempty >= 0:
        assert n_heavy <= n_nonempty <= n_rows
        n_light = n_nonempty - n_heavy
    n_wide = 0
    if light_rows and n_not_wide >= 0 and k["short_wide"] != 0:
        assert 1 <= wmax <= 32 and n_not_wide <= n_rows - n_heavy
        n_wide = max(0, n_light - n_not_wide)
    if not has_plan:
        n_heavy, th = 0, INT32_MAX
    n_hub = max(0, min(n_hub, n_heavy))
    if flags & NOHUB:
        n_heavy -= n_hub
        n_hub = 0
    hub_only = bool(flags & HUBONLY)
    if hub_only and n_hub == 0:
        return None
    lines = ldx % 32 == 0 and xa % 128 == 0
    hub_hc = k["hub_chunk"] if k["hub_chunk"] else (32 if lines and F <= 192 else 64)
    E["hub_chunk"] = hub_hc
    E["hub_loaders"] = 7 if k["hub_loaders"] == 7 else 15
    hub_deferred = False

    def hub_launch(mode):
        E["hub"] = mode
    if n_hub > 0:
        assert n_hub * ((F + 31) // 32) < INT32_MAX
        serial = k["hub_stream"] == 2 or (k["hub_stream"] == 0 and bool(flags & SERIAL))
        hub_deferred = serial and not hub_only and bool(k["hub_fuse"]) and k["hub_chunk"] == 0
        E["hub_n_chunks"] = (F + hub_hc - 1) // hub_hc
        E["hub_grid"] = n_hub * E["hub_n_chunks"]
        if not hub_deferred:
            hub_launch(1 if (not hub_only and not serial) else 2)
        n_heavy -= n_hub
        if hub_only:
            return E
    E["n_heavy"] = n_heavy
    F4 = (F + 3) // 4 * 4
    v4_ok = ldx % 4 == 0 and xa % 16 == 0 and F4 <= ldx and F4 >= 32 and (F4 == F or bool(flags & XP))
    pad_both = bool(flags & XP) and bool(flags & YP)
    F_csr = F4 if (F % 4 != 0 and pad_both and 128 < F4 <= 256 and F4 <= ldx and F4 <= ldy) else F
    csr_v4 = F_csr % 4 == 0 and pick_vec(k, F_csr, ldx, ldy, xa, ya) == 4
    small_wide = n_rows * F <= (1 << 23) and F > 256 and k["rows_per_wave"] == 0 and \
        k["slice_floats"] == 128
    wide_rows = n_rows >= 65536 and (F4 == 128 or F4 > 256)
    rows_kernel = v4_ok and k["rows_per_wave"] != 1 and not small_wide and \
        (k["rows_per_wave"] > 1 or not csr_v4 or F4 < 128 or wide_rows)
    hp = k["heavy_pairs"]
    if rows_kernel:
        E["multi_row"] = 1
        vec_store = int(ldy % 4 == 0 and ya % 16 == 0 and F4 <= ldy and (F4 == F or bool(flags & YP)))
        LR = (16 if k["rows_per_wave"] == 4 else 32) if F4 >= 128 else F4 // 4
        LR = min(LR, 32)
        SW = LR * 4
        multi = F4 > SW
        vh2 = F % 2 == 0 and ldx % 2 == 0 and ldy % 2 == 0 and xa % 8 == 0 and ya % 8 == 0 and \
            (not multi or SW % 128 == 0)
        assert n_heavy * 8 + n_rows < INT32_MAX
        fused = hub_deferred and LR >= 16 and vh2 and F4 > 64
        if hub_deferred and not fused:
            hub_launch(2)
        E["kernel"] = 2 if fused else 1
        o32 = bool(flags & U4G) and ldx * 4 < (1 << 24)
        qv = ((2 if F4 > 16 else 1) if ((hp & 4) and LR <= 16 and F4 <= 32) else 0)
        if (hp & 8) and LR <= 16 and 32 < F4 <= 64:
            qv = 4
        wide = n_wide > 0 and LR == 32 and multi and not fused and qv == 0 and \
            (k["short_wide"] > 0 or n_rows >= 65536)
        E.update(O32=int(o32), LR=LR, F_load=F4, vec_store=vec_store, kernel_bits=hp & 17)
        R = 64 // LR
        if wide:
            VH = 2 if vh2 else 1
            WD = 16 if wmax <= 16 else 32
            slices = (F4 + SW - 1) // SW
            n_sub = 1 if (hp & 1) else SW // (64 * VH)
            n_narrow = n_light - n_wide
            waves = n_heavy * n_sub + (n_narrow + R - 1) // R
            slice_blocks = (waves + 3) // 4
            wide_blocks = ((n_wide + R - 1) // R + 3) // 4
            blocks = slice_blocks * slices + wide_blocks
            assert blocks < INT32_MAX and n_narrow >= 0
            E.update(LB=16, VH=VH, QV=0, HF=0, WD=WD, slices=slices, n_sub=n_sub,
                     n_light_items=n_narrow, n_wide=n_wide, wide_first=k["short_wide_first"],
                     slice_blocks=slice_blocks, wide_blocks=wide_blocks, grid_x=blocks, grid_y=1)
            return E
        if qv == 4:
            LB, VH, QV, HF = (16 if LR >= 16 else 8), 2, 4, 0
        elif qv == 2:
            LB, VH, QV, HF = 8, 2, 2, 0
        elif qv == 1:
            LB, VH, QV, HF = 8, 2, 1, 0
        elif fused:
            LB, VH, QV, HF = 16, 2, 0, 32
        elif LR >= 16:
            LB, VH, QV, HF = 16, (2 if vh2 else 1), 0, 0
        else:
            LB, VH, QV, HF = 8, (2 if vh2 else 1), 0, 0
        assert LR > 0 and R * LB <= 64
        slices = (F4 + SW - 1) // SW
        n_sub = 1 if (QV > 0 or (hp & 1)) else (SW // (64 * VH) if slices > 1 else
                                                (F4 + 64 * VH - 1) // (64 * VH))
        n_items = n_light if light_rows else n_rows
        waves = n_heavy * n_sub + (n_items + R - 1) // R
        hub_chunks = (F + 31) // 32 if fused else 0
        n_hub_blocks = n_hub * hub_chunks if fused else 0
        blocks = (waves + 3) // 4 + n_hub_blocks
        assert blocks < INT32_MAX
        if fused:
            E["hub"] = 3
        E.update(LB=LB, VH=VH, QV=QV, HF=HF, slices=slices, n_sub=n_sub, n_light_items=n_items,
                 grid_x=blocks, grid_y=slices, fused_chunks=hub_chunks, fused_blocks=n_hub_blocks)
        return E
    V = pick_vec(k, F_csr, ldx, ldy, xa, ya)
    aF = F_csr if V == 4 else F
    chunks_total = (aF + 64 * V - 1) // (64 * V)
    cmax = 16 // V
    sf = 512 if small_wide else k["slice_floats"]
    C = max(1, sf // (64 * V)) if sf > 0 else cmax
    C = min(C, cmax, chunks_total)
    slices = (chunks_total + C - 1) // C
    assert n_heavy * C * V + n_rows < INT32_MAX and slices < 65536
    fused = hub_deferred and V == 4 and C == 1
    if hub_deferred and not fused:
        hub_launch(2)
    hub_chunks = (F + 31) // 32 if fused else 0
    n_hub_blocks = n_hub * hub_chunks if fused else 0
    VH = min(2, V)
    waves = n_heavy * (C * V // VH) + n_rows
    blocks = (waves + 3) // 4 + n_hub_blocks
    if fused:
        E["hub"] = 3
    E.update(kernel=3 if fused else 0, V=V, C=C, VH=VH, HF=32 if fused else 0, F_load=aF,
             slices=slices, n_sub=C * V // VH, n_light_items=n_rows, grid_x=blocks, grid_y=slices,
             kernel_bits=((hp >> 1) & 1) | (2 if n_rows >= (1 << 20) else 0),
             fused_chunks=hub_chunks, fused_blocks=n_hub_blocks)
    return E


EF = ["kernel", "multi_row", "V", "C", "LB", "VH", "QV", "HF", "WD", "O32", "LR", "F_load",
      "vec_store", "slices", "n_sub", "n_heavy", "n_light_items", "n_wide", "wide_first",
      "slice_blocks", "wide_blocks", "grid_x", "grid_y", "kernel_bits", "hub", "hub_chunk",
      "hub_loaders", "hub_n_chunks", "hub_grid", "fused_chunks", "fused_blocks"]
rows = []


def case(name, n_rows, F, ldx, ldy, xa, ya, flags, plan, k=None):
    kk = dict(DEF)
    kk.update(k or {})
    has_plan, n_heavy, n_hub, th, ne, nnw, wmax = plan
    E = parent(n_rows, F, ldx, ldy, xa, ya, flags, has_plan, n_heavy, n_hub, th, ne, nnw, wmax, kk)
    assert E is not None, name
    rows.append('{"%s",%d,%d,%d,%d,0x%xull,0x%xull,%du,%d,%d,%d,%d,%d,%d,%d,{%s},{%s}},'
                % (name, n_rows, F, ldx, ldy, xa, ya, flags, int(has_plan), n_heavy, n_hub, th, ne, nnw,
                   wmax, ",".join(str(kk[x]) for x in KN), ",".join(str(E[x]) for x in EF)))


BASE = 0x7f0000000000  # a 2 MiB-aligned allocation

# ---- the benchmark shapes -------------------------------------------------------------
NR = 232965
for yname, ldy, yf in (("padded", 608, YP), ("contig", 602, 0)):
    for acc in (0, ACC):
        for nnw, wmax in ((-1, 0), (150000, 16)):
            case("reddit_%s_%s_%s" % (yname, "acc" if acc else "plain", "wide" if wmax else "nowide"),
                 NR, 602, 608, ldy, BASE, BASE + (1 << 30), XP | yf | U4G | ORDER | acc,
                 (True, 11234, 37, 512, 230100, nnw, wmax))
case("rmat_4g", 1 << 22, 256, 256, 256, BASE, BASE + (1 << 33), XP | YP | ORDER,
     (True, 61234, 511, 512, (1 << 22) - 1000, 3000000, 16))
case("rmat_4g_last_hop_acc", 1 << 22, 256, 256, 256, BASE, BASE + (1 << 33), XP | ORDER | ACC,
     (True, 20000, 100, 512, 3000000, 2000000, 16))
case("pubmed_serial_hub", 19717, 500, 512, 512, BASE, BASE + (1 << 26), XP | YP | U4G | ORDER | SERIAL,
     (True, 12, 3, 64, 19717, 700, 16))
case("pubmed_serial_hub_contig_out", 19717, 500, 512, 500, BASE, BASE + (1 << 26),
     XP | U4G | ORDER | SERIAL, (True, 12, 3, 64, 19717, 700, 16))
case("pubmed_serial_hub_nofuse", 19717, 500, 512, 512, BASE, BASE + (1 << 26),
     XP | YP | U4G | ORDER | SERIAL, (True, 12, 3, 64, 19717, 700, 16), dict(hub_fuse=0))
case("cora_contig", 2708, 1433, 1433, 1433, BASE, BASE + (1 << 26), U4G | ORDER,
     (True, 5, 0, 64, 2708, 300, 16))
case("cora_lines", 2708, 1433, 1440, 1440, BASE, BASE + (1 << 26), XP | YP | U4G | ORDER,
     (True, 5, 0, 64, 2708, 300, 16))
for P, w in ((2, 304), (4, 146), (8, 76)):
    ld = (w + 31) // 32 * 32
    case("reddit_block_P%d" % P, NR, w, ld, ld, BASE, BASE + (1 << 30), XP | YP | U4G | ORDER,
         (True, 11234, 37, 512, 230100, 150000, 16))
    case("reddit_block_P%d_last_hop" % P, NR, w, ld, 602, BASE, BASE + (1 << 30) + 4 * w,
         XP | U4G | ORDER, (True, 11234, 37, 512, 230100, 150000, 16))

# ---- the IEEE suite's graph (tests/ieee_operands.py, N = 4096) and a large twin ----------
import ieee_operands as io
N = 4096
deg = np.diff(io.edge_graph(N, 0, "wild").row_ptr)


def plan_of(th, hub, ts, d=deg, scale=1):
    hub = max(hub, th)
    nh, nhub = int((d > th).sum()) * scale, int((d > hub).sum()) * scale
    n = len(d) * scale
    serial = nhub > 0 and int(d.max()) <= 3072
    fl = (SERIAL if serial else 0) | (ORDER if n > nh else 0)
    ne = int((d > 0).sum()) * scale
    nnw, wmax = (-1, 0) if ts <= 0 or not (n > nh) else (max(0, int((d > ts).sum()) * scale - nh), ts)
    return fl, (True, nh, nhub, th, ne, nnw, wmax)


def layout(how, F):
    if how == "lines":
        return (F + 31) // 32 * 32 + 32, 0, XP | YP
    if how == "contig":
        return F, 0, 0
    return F + 7, 3, 0


def ieee(tag, F, how, th, hub, k, n_scale=1, extra=0):
    kk = dict(DEF)
    kk.update(k)
    ts = 16 if kk["short_wide"] < 0 else kk["short_wide"]
    fl, plan = plan_of(th, hub, ts, scale=n_scale)
    ld, off, lf = layout(how, F)
    n = N * n_scale
    u4g = U4G if n < (1 << 24) and n * ld * 4 < (1 << 32) else 0
    case("%s/%d%s/%d" % (tag, F, how[0], len(rows)),
         n, F, ld, ld, BASE + 4 * off, BASE + (1 << 30) + 4 * off, lf | u4g | fl | extra, plan, k)


WIDTHS = [1, 3, 12, 30, 32, 33, 64, 65, 130, 152, 256, 602]
for F in WIDTHS:
    for how in ("lines", "contig", "slice"):
        for rpw in (0, 1, 2, 4):
            ieee("rpw", F, how, 40, 500, dict(rows_per_wave=rpw))
        ieee("light", F, how, 10**9, 10**9, {})
        ieee("rpw_big", F, how, 40, 500, {}, n_scale=32)
for F, how, rpw in [(30, "lines", 0), (32, "contig", 0), (33, "lines", 0), (64, "contig", 0),
                    (65, "lines", 0), (130, "lines", 2), (602, "lines", 2), (152, "contig", 1),
                    (256, "lines", 0), (3, "slice", 0)]:
    for hp in (0, 1, 5, 13, 17, 29, 31):
        ieee("hp", F, how, 16, 200, dict(rows_per_wave=rpw, heavy_pairs=hp))
for F, how in [(64, "lines"), (130, "lines"), (152, "lines"), (65, "slice"), (602, "lines")]:
    for hc in (0, 32, 64):
        for stream in (0, 1, 2):
            for fuse in (0, 1):
                # (hub_loaders only picks spmm_hub_kernel's second argument: 7 once per chunk)
                ieee("hub", F, how, 16, 200, dict(hub_chunk=hc, hub_loaders=7 if stream == fuse else 15,
                                                  hub_stream=stream, hub_fuse=fuse))
for F, how in [(130, "lines"), (152, "contig"), (256, "lines"), (602, "lines")]:
    for sw in (-1, 0, 16, 32):
        for scale in (1, 32):  # 4,096 rows and 131,072 (>= 65,536: the rule applies)
            for rpw, fuse in ((2, 0), (0, 1)):
                # (short_wide_first is passed through: 1 with the forced multi-row kernel)
                ieee("wide", F, how, 40, 500, dict(rows_per_wave=rpw, hub_fuse=fuse, short_wide=sw,
                                                    short_wide_first=int(rpw == 2)), n_scale=scale)
            ieee("wide_acc", F, how, 40, 500, dict(rows_per_wave=2, hub_fuse=0, short_wide=sw),
                 n_scale=scale, extra=ACC)
# split launches
ieee("nohub", 130, "lines", 16, 200, {}, extra=NOHUB)
ieee("hubonly", 130, "lines", 16, 200, {}, extra=HUBONLY)
ieee("hubonly", 602, "slice", 16, 200, dict(hub_loaders=7), extra=HUBONLY)

open(os.path.join(ROOT, "tests", "spmm_schedule_cases.inc"), "w").write(
    "// Expected schedules: literals derived once from launch_spmm as it stood before\n"
    "// spmm_schedule.h existed (commit 4ee6fe1), not from spmm_schedule().  Columns:\n"
    "// name, n_rows, F, ldx, ldy, X, Y, flags, plan?, n_heavy, n_hub, threshold, n_nonempty,\n"
    "// n_not_wide, wide_max_nnz, {knobs in SpmmKnobs order}, {SpmmSchedule in field order}\n"
    + "\n".join(rows) + "\n")
print(len(rows), "cases")
