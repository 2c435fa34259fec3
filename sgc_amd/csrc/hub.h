// hub.h -- the LDS-staged hub-row work item (hub_body) shared by the fp32 SpMM
// kernels (spmm.hip) and the 16-bit-feature kernels (spmm16.hip).
#pragma once

#include "common.h"
#include "lane_lines.h"
#include "x16.h"

namespace sgc {

// ---------------------------------------------------------------------------
// Hub rows (degree > hub_threshold): one 1024-thread workgroup per (row,
// HC-feature chunk).  A single wave's FMA chain over d nonzeros costs d FMAs
// -- cheap -- but a wave keeps only ~16 nonzeros' X segments in flight, so a
// 48k-nonzero hub on one wave runs ~3 ms, longer than a whole hop at P >= 2
// GPUs.  Here 15 loader waves gather X segments into an LDS double buffer
// while wave 0 runs the sequential chain out of LDS -- the same FMA order.
//
// The chain is the block's floor, so:
//  * wave 0 reads four nonzeros' X values per lane with one ds_read_b128 and
//    their four values with one broadcast ds_read_b128: the staging image is
//    transposed, gxT[feature][nonzero], row stride kStride = 4 mod 64 dwords
//    (conflict-free b128 reads per 16-lane group and b128 writes per 8-lane
//    group); each loader lane holds 16 CONSECUTIVE nonzeros of its feature
//    and writes them with four ds_write_b128;
//  * loaders keep kHubDepth rounds in registers: round t+kHubDepth is issued
//    while round t+1 is written, so a load has kHubDepth-1 rounds of FMA time
//    to land (a round is ~0.5 us of chain; an HBM/IC gather ~1-2 us), and the
//    column ids of a round arrive one round before its X loads.
// HC = 32 (one 128-B line per nonzero; lanes 32-63 load the second 16
// nonzeros of the loader's run) halves the bytes each block ingests per
// nonzero and spreads a hub over twice the CUs; it needs 128-B aligned X rows
// to stay one line per segment.
constexpr int kHubInstr = 16;  // consecutive nonzeros per loader lane per round
constexpr int kHubDepth = 3;   // rounds held in loader registers (17 loads each: vmcnt <= 63)
constexpr int kHubUnroll = 6;  // lcm(kHubDepth, 2): X ring slot and colv parity compile-time
constexpr int kHubPre = 4;     // LDS batches of 4 nonzeros the chain reads ahead

// The fused rows + hub launches (hub_body<HF, 3> inside spmm_csr_kernel /
// spmm_rows_kernel) stage IN = 8 nonzeros per loader lane: their LDS image is
// 18 KB instead of 35 KB, and since every workgroup of a launch carries it,
// eight workgroups (32 waves) fit a CU instead of four -- the light rows of a
// small graph are latency-bound and need the occupancy (Pubmed shape: the
// light rows alone ran 30.5 us per hop, fused at 35 KB 37.5 us).
template <int HC, int NL, int IN = kHubInstr>
struct HubShape {
    static_assert(IN % 4 == 0 && IN <= kHubInstr, "loader run: whole b128 LDS writes");
    static constexpr int kSegs = kWave / HC;                     // nonzero runs per loader wave
    static constexpr int kPerLoader = IN * kSegs;                // nonzeros per loader per round
    static constexpr int kRound = NL * kPerLoader;  // nonzeros per round (240 / 480 at NL = 15)
    static constexpr int kPad = 4 * kHubPre;        // read-ahead past kRound
    // dwords per gxT row: 4 mod 64 (conflict-free b128), and >= kRound + kPad
    // for the FMA loop's read-ahead (kHubPre batches of 4 past the last full batch)
    static constexpr int kStride = (kRound + kPad + 63) / 64 * 64 + 4;
};

#ifndef SGC_HUB_STAMPS
#define SGC_HUB_STAMPS 0  // diagnostic build only: per-round clock stamps of block 0
#endif
#if SGC_HUB_STAMPS
// [0] chain wave leaves the round's barrier, [1] chain wave reaches the next
// barrier (FMAs done), [2] loader wave 1 after its LDS store, [3] loader wave
// 1 reaches the barrier (loads issued); [4][0..1] s_memtime / s_memrealtime
// at kernel start and end (clock rate).  Lane 0's vector stores only; read
// back with sgc_debug_hub_stamps (exported by this build only).
constexpr int kStampRounds = 4096;
__device__ unsigned long long g_hub_stamp[5][kStampRounds];
#define HUB_STAMP(slot, r)                                                            \
    do {                                                                              \
        if (bid == 0 && lane == 0 && (r) < kStampRounds)                              \
            g_hub_stamp[slot][r] = __builtin_amdgcn_s_memtime();                      \
    } while (0)
#else
#define HUB_STAMP(slot, r) \
    do {                   \
    } while (0)
#endif

// The chain with the S values off the LDS-read path: one ds_read_b32 per 16
// nonzeros (lane l reads v[16i + (l & 15)], so each 16-lane row holds the
// iteration's 16 values) and every FMA takes its S value by a DPP row
// broadcast (v_fmac_f32_dpp ... row_newbcast:k): four LDS reads per 16
// nonzeros instead of eight.  Same operands and order as hub_chain_asm:
// acc = fma(v[k], x[k], acc).  X ring of four b128 slots (v80..v95) read four
// batches ahead; S in v96 (even iterations) / v97 (odd), read two iterations
// ahead (gv carries 32 floats of padding for it).  Invariant at the top of an
// iteration: outstanding LDS reads = [S_i, X0..X3, S_i+1].
__device__ __forceinline__ void hub_chain_dpp(float &acc, uint32_t xa, uint32_t vl, int iters,
                                              int rem) {
    asm volatile(
        "s_waitcnt lgkmcnt(0)\n"
        "ds_read_b32 v96, %[vl]\n"
        "ds_read_b128 v[80:83], %[xa]\n"
        "ds_read_b128 v[84:87], %[xa] offset:16\n"
        "ds_read_b128 v[88:91], %[xa] offset:32\n"
        "ds_read_b128 v[92:95], %[xa] offset:48\n"
        "ds_read_b32 v97, %[vl] offset:64\n"
        "s_cmp_eq_u32 %[it], 0\n"
        "s_cbranch_scc1 2f\n"
        "1:\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v96, v80 row_newbcast:0 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v81 row_newbcast:1 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v82 row_newbcast:2 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v83 row_newbcast:3 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[80:83], %[xa] offset:64\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v96, v84 row_newbcast:4 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v85 row_newbcast:5 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v86 row_newbcast:6 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v87 row_newbcast:7 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[84:87], %[xa] offset:80\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v96, v88 row_newbcast:8 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v89 row_newbcast:9 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v90 row_newbcast:10 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v91 row_newbcast:11 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[88:91], %[xa] offset:96\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v96, v92 row_newbcast:12 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v93 row_newbcast:13 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v94 row_newbcast:14 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v95 row_newbcast:15 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[92:95], %[xa] offset:112\n"
        "ds_read_b32 v96, %[vl] offset:128\n"
        "v_add_u32 %[xa], 64, %[xa]\n"
        "v_add_u32 %[vl], 64, %[vl]\n"
        "s_sub_u32 %[it], %[it], 1\n"
        "s_cmp_eq_u32 %[it], 0\n"
        "s_cbranch_scc1 3f\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v97, v80 row_newbcast:0 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v81 row_newbcast:1 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v82 row_newbcast:2 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v83 row_newbcast:3 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[80:83], %[xa] offset:64\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v97, v84 row_newbcast:4 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v85 row_newbcast:5 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v86 row_newbcast:6 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v87 row_newbcast:7 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[84:87], %[xa] offset:80\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v97, v88 row_newbcast:8 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v89 row_newbcast:9 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v90 row_newbcast:10 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v91 row_newbcast:11 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[88:91], %[xa] offset:96\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v97, v92 row_newbcast:12 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v93 row_newbcast:13 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v94 row_newbcast:14 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v95 row_newbcast:15 row_mask:0xf bank_mask:0xf\n"
        "ds_read_b128 v[92:95], %[xa] offset:112\n"
        "ds_read_b32 v97, %[vl] offset:128\n"
        "v_add_u32 %[xa], 64, %[xa]\n"
        "v_add_u32 %[vl], 64, %[vl]\n"
        "s_sub_u32 %[it], %[it], 1\n"
        "s_cmp_lg_u32 %[it], 0\n"
        "s_cbranch_scc1 1b\n"
        // even count done: the next iteration's S is in v96
        "2:\n"
        "s_cmp_gt_u32 %[rem], 0\n"
        "s_cbranch_scc0 5f\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v96, v80 row_newbcast:0 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v81 row_newbcast:1 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v82 row_newbcast:2 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v83 row_newbcast:3 row_mask:0xf bank_mask:0xf\n"
        "s_cmp_gt_u32 %[rem], 1\n"
        "s_cbranch_scc0 5f\n"
        "s_waitcnt lgkmcnt(3)\n"
        "v_fmac_f32_dpp %[acc], v96, v84 row_newbcast:4 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v85 row_newbcast:5 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v86 row_newbcast:6 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v87 row_newbcast:7 row_mask:0xf bank_mask:0xf\n"
        "s_cmp_gt_u32 %[rem], 2\n"
        "s_cbranch_scc0 5f\n"
        "s_waitcnt lgkmcnt(2)\n"
        "v_fmac_f32_dpp %[acc], v96, v88 row_newbcast:8 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v89 row_newbcast:9 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v90 row_newbcast:10 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v96, v91 row_newbcast:11 row_mask:0xf bank_mask:0xf\n"
        "s_branch 5f\n"
        // odd count done: the next iteration's S is in v97
        "3:\n"
        "s_cmp_gt_u32 %[rem], 0\n"
        "s_cbranch_scc0 5f\n"
        "s_waitcnt lgkmcnt(4)\n"
        "v_fmac_f32_dpp %[acc], v97, v80 row_newbcast:0 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v81 row_newbcast:1 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v82 row_newbcast:2 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v83 row_newbcast:3 row_mask:0xf bank_mask:0xf\n"
        "s_cmp_gt_u32 %[rem], 1\n"
        "s_cbranch_scc0 5f\n"
        "s_waitcnt lgkmcnt(3)\n"
        "v_fmac_f32_dpp %[acc], v97, v84 row_newbcast:4 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v85 row_newbcast:5 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v86 row_newbcast:6 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v87 row_newbcast:7 row_mask:0xf bank_mask:0xf\n"
        "s_cmp_gt_u32 %[rem], 2\n"
        "s_cbranch_scc0 5f\n"
        "s_waitcnt lgkmcnt(2)\n"
        "v_fmac_f32_dpp %[acc], v97, v88 row_newbcast:8 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v89 row_newbcast:9 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v90 row_newbcast:10 row_mask:0xf bank_mask:0xf\n"
        "v_fmac_f32_dpp %[acc], v97, v91 row_newbcast:11 row_mask:0xf bank_mask:0xf\n"
        "s_branch 5f\n"
        "5:\n"
        "s_waitcnt lgkmcnt(0)\n"
        : [acc] "+v"(acc), [xa] "+v"(xa), [vl] "+v"(vl), [it] "+s"(iters)
        : [rem] "s"(rem)
        : "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91",
          "v92", "v93", "v94", "v95", "v96", "v97", "scc", "memory");
}

// NL loader waves + the chain wave per workgroup: 15 (1024 threads, ~133 KB
// of LDS: one workgroup per CU) or 7 (512 threads, ~68 KB: two per CU, half
// the CU held per hub chain; sgc_set_tuning("hub_loaders")).
// The body of one hub work item (hub row h, feature chunk c of block `bid`),
// shared by spmm_hub_kernel and the fused rows + hub launch of
// spmm_rows_kernel (HF > 0: NL = 3, the rows kernel's 256 threads).
// XT / YT: the element types of X and Y in memory (float, or bf16_t / f16_t
// of x16.h: the loaders widen each gathered element as they stage it, so the
// LDS image and the chain are the fp32 ones, and the final store rounds once).
template <int HC, int NL, int IN, typename XT = float, typename YT = float>
__device__ __forceinline__ void hub_body(
    int bid, const int *__restrict__ row_ptr, const int *__restrict__ col,
    const float *__restrict__ val, const XT *__restrict__ X, int64_t ldx,
    YT *__restrict__ Y, int64_t ldy, int row_begin, int F, const int *__restrict__ hub_rows,
    int n_chunks, int accum) {
    using Sh = HubShape<HC, NL, IN>;
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float gxT[2][HC * Sh::kStride];  // 2 x 66.5 KB
    __shared__ __attribute__((aligned(16)))
    float gv[2][Sh::kRound + Sh::kPad + 32];  // + the DPP chain's S read-ahead
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    // wave 0 runs the chain, waves 1..NL load (loader index li)
    const bool loader = w > 0;
    const int li = w - 1;
    const int h = bid / n_chunks;
    const int c = bid - h * n_chunks;
    const int row = hub_rows[h];
    const int k0 = row_ptr[row], k1 = row_ptr[row + 1];
    const int fl = lane & (HC - 1);  // feature within the chunk
    const int seg = lane / HC;       // which run of IN nonzeros (HC = 32: 0 or 1)
    const int f = c * HC + fl;
    // lanes beyond F gather column F - 1: a line the chunk's active lanes read
    const uint32_t boff = (uint32_t)gather_col(f, F, 1) * (uint32_t)sizeof(XT);
    const char *Xb = reinterpret_cast<const char *>(X);
    const int64_t row_bytes = ldx * (int64_t)sizeof(XT);
    const int n_round = (k1 - k0 + Sh::kRound - 1) / Sh::kRound;
    const int my_k = lane & (Sh::kPerLoader - 1);  // this lane's nonzero of the loader's run
    float regs[kHubDepth][IN];
    float vreg[kHubDepth];
    int colv[2];  // column ids of the loader's run, one per lane, for two future rounds
    // Loader waves only; `s` and `p` are compile-time constants after unrolling.
    // Column ids come in with ONE coalesced load per round (lane j holds
    // nonzero j's id, broadcast with v_readlane), issued a round before the X
    // loads that use them (per-nonzero scalar loads, each waited on, cost
    // ~0.4 us per round: 493 -> 406 us on the 47,857-nonzero row).
    auto load_col = [&](int r, int p) {
        const int kr = k0 + r * Sh::kRound + li * Sh::kPerLoader;
        colv[p] = col[min(kr + my_k, k1 - 1)];
    };
    auto load_x = [&](int r, int s, int p) {
        const int kr = k0 + r * Sh::kRound + li * Sh::kPerLoader;
#pragma unroll
        for (int j = 0; j < IN; ++j) {
            int cj = __builtin_amdgcn_readlane(colv[p], j);
            if (HC == 32) {
                const int c1 = __builtin_amdgcn_readlane(colv[p], IN + j);
                cj = seg ? c1 : cj;
            }
            regs[s][j] = load_elem<XT>(Xb + (int64_t)cj * row_bytes + boff);
        }
        vreg[s] = val[min(kr + my_k, k1 - 1)];
    };
    auto store = [&](int buf, int s) {
        f4 *dst = reinterpret_cast<f4 *>(
            &gxT[buf][fl * Sh::kStride + li * Sh::kPerLoader + seg * IN]);
#pragma unroll
        for (int q = 0; q < IN / 4; ++q)
            dst[q] = f4{regs[s][4 * q], regs[s][4 * q + 1], regs[s][4 * q + 2], regs[s][4 * q + 3]};
        if (lane < Sh::kPerLoader) gv[buf][li * Sh::kPerLoader + lane] = vreg[s];
    };
    // Loads are never predicated (rounds past the row re-read its last
    // nonzero): a conditional load makes its registers a phi, and copying a
    // phi waits for every load in flight.
    if (loader) {
#pragma unroll
        for (int s = 0; s < kHubDepth; ++s) {
            load_col(s, s & 1);
            load_x(s, s, s & 1);
        }
        load_col(kHubDepth, kHubDepth & 1);
        if (n_round > 0) store(0, 0);
    }
#if SGC_HUB_STAMPS
    if (bid == 0 && threadIdx.x == 0) {
        g_hub_stamp[4][0] = __builtin_amdgcn_s_memtime();
        g_hub_stamp[4][1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    __syncthreads();
    float acc = 0.0f;
    if constexpr (sizeof(YT) == 4) {  // (a chain is never continued from a rounded store)
        if (accum && w == 0 && f < F) acc = load_elem<YT>(Y + (int64_t)(row - row_begin) * ldy + f);
    }
    for (int r0 = 0; r0 < n_round; r0 += kHubUnroll) {
#pragma unroll
        for (int s = 0; s < kHubUnroll; ++s) {
            // round t's X lives in regs[t % kHubDepth], its column ids in colv[t & 1]
            const int r = r0 + s;
            if (r >= n_round) break;  // block-uniform
            const int buf = r & 1;
            if (w == 0) HUB_STAMP(0, r);
            if (loader) {
                if (r + 1 < n_round) store(buf ^ 1, (s + 1) % kHubDepth);
                if (w == 1) HUB_STAMP(2, r);
                // ids of round r+D+1 first, so waiting for them (next round)
                // does not also wait for this round's X loads
                load_col(r + kHubDepth + 1, (s + kHubDepth + 1) & 1);
                load_x(r + kHubDepth, s % kHubDepth, (s + kHubDepth) & 1);
            } else if (w == 0) {
                const int n = min(Sh::kRound, k1 - (k0 + r * Sh::kRound));
                const int n4 = n >> 2;
                // LDS reads run kPre batches of four nonzeros ahead of the FMA
                // chain (a ds_read's ~64-cycle latency otherwise lands on the
                // chain every four FMAs); reads past n stay inside the padded
                // row / value buffers (kStride, gv) and are never used.
                // The chain as one asm loop (hub_chain_dpp): X values read
                // four batches of four nonzeros ahead with counted lgkmcnt
                // waits (left to the compiler the reads sink to one batch
                // ahead), the round's S values by one ds_read_b32 per 16
                // nonzeros and a DPP row broadcast per FMA.  Same FMA order.
                // What bounds it is one wave's LDS read rate: ~35 cycles per
                // 1-KB ds_read_b128 on gfx950 (scripts/micro/fma_chain.hip:
                // 9.5 cycles per nonzero alone, ~14-16 beside the loaders' LDS
                // writes; profiles/r02/micro_fma_chain_v2.log, hub_stamps.log).
                typedef __attribute__((address_space(3))) const float lds_f;
                const uint32_t xa = (uint32_t)(size_t)(lds_f *)(&gxT[buf][fl * Sh::kStride]);
                const uint32_t vl = (uint32_t)(size_t)(lds_f *)(&gv[buf][lane & 15]);
                hub_chain_dpp(acc, xa, vl, n4 >> 2, n4 & 3);
                const float *xt = &gxT[buf][fl * Sh::kStride];
                for (int kk = n4 * 4; kk < n; ++kk) acc = __builtin_fmaf(gv[buf][kk], xt[kk], acc);
            }
            if (w == 0) HUB_STAMP(1, r);
            if (w == 1) HUB_STAMP(3, r);
            __syncthreads();
        }
    }
    if (w == 0 && seg == 0 && f < F) store_elem<YT>(Y + (int64_t)(row - row_begin) * ldy + f, acc);
#if SGC_HUB_STAMPS
    if (bid == 0 && threadIdx.x == 0) {
        g_hub_stamp[4][2] = __builtin_amdgcn_s_memtime();
        g_hub_stamp[4][3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

}  // namespace sgc
