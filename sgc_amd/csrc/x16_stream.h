// x16_stream.h -- what the kernels of the 16-bit classifier share (linear16.hip,
// xent16.hip, eval16.hip): namespace x16's helpers, the one streaming GEMM of
// the three forwards, and the body of the weight backward's two forms.
//
// x16::stream is the forward of linear_x16_kernel, xent_fwd_x16_kernel and
// eval_fwd_x16_kernel up to the end of a tile; each kernel passes what it does
// with a finished tile (store or hold it, softmax + G + loss, argmax + loss).
// x16::dw_cols is the weight backward; xent_dw_cols_x16_kernel (linear16.hip)
// and xent_dw_cols_x16_stop_kernel (xent16.hip) are thin wrappers, each in
// its own unit (a second set of kernels in one unit has changed the register
// allocation of the first: see xent.hip).
#pragma once

#include <algorithm>

#include "gemm_tile.h"
#include "internal.h"
#include "split_bf16.h"
#include "x16.h"

namespace sgc {
namespace x16 {

template <int U> struct SlotC { static constexpr int value = U; };
template <int U, int D, typename F>
__device__ __forceinline__ void each_slot(F &&f) {
    if constexpr (U < D) {
        f(SlotC<U>{});
        each_slot<U + 1, D>(f);
    }
}
template <int U, int D, typename F>
__device__ __forceinline__ bool run_slots(F &&f) {
    if constexpr (U < D) {
        if (!f(SlotC<U>{})) return false;
        return run_slots<U + 1, D>(f);
    } else {
        return true;
    }
}

__device__ __forceinline__ uint32_t ror8(uint32_t x) {  // lane j of each 16-lane row gets lane j ^ 8's x
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false);
}

// Two 16-bit elements of one dword (a in the low half) as packed bf16 pieces
// with a == h + m exactly: bf16 is its own piece (m unused), fp16 widens
// (v_cvt_f32_f16), rounds to bf16 (v_cvt_pk_bf16_f32) and subtracts once.
template <typename XT>
__device__ __forceinline__ void pieces16(uint32_t w, uint32_t &h, uint32_t &m) {
    if constexpr (sizeof(XT) == 2 && __is_same(XT, bf16_t)) {
        h = w;
        m = 0u;
    } else {
        float a, b;
        widen16x2<f16_t>(w, a, b);
        h = pk_bf16(a, b);
        m = pk_bf16(a - __uint_as_float(h << 16), b - __uint_as_float(h & 0xffff0000u));
    }
}

constexpr int kDepth = 4;  // 64-k double chunks in flight per wave (the fp32 ring's bytes)
constexpr int kHeld = 6;   // finished tiles held per wave at NT <= 3 (four at NT = 4)
constexpr int kWaves = 8;

// W image geometry (host and device): bytes per 32-k half chunk for NT class
// tiles, the last holding Cl classes (the layout of linear_split_kernel).
__host__ __device__ constexpr int chunk_bytes(int NT, int Cl) {
    return (NT - 1) * 3072 + (4 * Cl + 1) * 48;
}
// Half chunks of the image: two per 64-k double chunk; the last double
// chunk's second half (k = 64c + 16kg + 8 .. + 15) lies wholly past K when at
// most 8 k remain, and is left out.
__host__ __device__ constexpr int half_chunks(int K) {
    return 2 * ((K + 63) / 64) - ((K - 1) % 64 < 8 ? 1 : 0);
}
// The layout is the contract between the image builder and the MFMA loop of
// stream(): a lane's granule (3 pieces x 16 B) per class of a full tile, the
// last tile's Cl classes x 4 k groups and its zero granule; a half chunk
// exists exactly when one of its k lies below K.
static_assert(chunk_bytes(1, 1) == 5 * 48 && chunk_bytes(1, 16) == 65 * 48, "last tile + zero granule");
static_assert(chunk_bytes(4, 16) == 3 * 3072 + 65 * 48 && chunk_bytes(3, 9) == 2 * 3072 + 37 * 48,
              "64 lanes x 48 B per full tile");
static_assert(half_chunks(1) == 1 && half_chunks(8) == 1 && half_chunks(9) == 2, "first double chunk");
static_assert(half_chunks(64) == 2 && half_chunks(65) == 3 && half_chunks(66) == 3, "second double chunk");
static_assert(half_chunks(72) == 3 && half_chunks(73) == 4 && half_chunks(128) == 4, "its second half");

// Dynamic LDS of a forward launch: the image and the tile counter.
inline size_t image_lds(int64_t K, int C) {
    const int NT = (C + 15) / 16;
    return (size_t)half_chunks((int)K) * chunk_bytes(NT, C - (NT - 1) * 16) + 16;
}

// The persistent grid of a forward kernel: its 160 KB dynamic-LDS attribute
// raised, one workgroup per CU, at most one per 16-row tile.
inline hipError_t persistent_grid(const void *kernel, int M, int *blocks) {
    int cus = 0;
    const hipError_t e = persistent_setup(kernel, &cus);
    *blocks = std::max(1, std::min(cus, (M + 15) / 16));
    return e;
}

// ---------------------------------------------------------------------------
// The forward stream, modelled on linear_split_kernel: persistent (one
// workgroup per CU), W's three-piece operand image built in-kernel behind the
// first X loads, a ring of compile-time slots, every load issued on every
// path (the counted waits stay exact), bias added at the end of a tile.
// * X stream: the shape that measured 5.5-5.8 TB/s -- 128 contiguous bytes of
//   each of 8 rows per wave-instruction, at 16 bits 64 k.  Per 16-row, 64-k
//   double chunk lane (j, kg) = (l & 15, l >> 4) issues two b128 loads: rows
//   j & 7 and 8 + (j & 7), segment 2 kg + (j >> 3).  The row_ror:8 exchange
//   leaves lane (j, kg) with k = 16 kg .. 16 kg + 15 of row j: two B operands
//   of v_mfma_f32_16x16x32_bf16 as they stand (bf16; no v_perm).  The
//   contraction order is free because the W image is built to match: the
//   granule of lane kg in MFMA q of double chunk c is k = 64c + 16kg + 8q.
// * k >= K of the ragged double chunk is zeroed in registers (the padding may
//   hold NaN); offsets past the tensor read 0 through the descriptor.
// * No M threshold: there is no 16-bit LDS-tile kernel to fall back on.
//
// lds: the kernel's dynamic LDS (image_lds bytes).  When a tile finishes,
// tile_end(tile, z) gets its number and z[n] = accH[n] + accL[n] + bias[n]:
// lane (j, kg) holds row j of the tile, classes 16 n + 4 kg + r (n < NT,
// r < 4); z is the callable's to change.  The waves take tiles dynamically,
// so which wave ends which tile differs run to run.
template <int NT, int NW, typename XT, typename TileEnd>
__device__ __forceinline__ void stream(char *const lds, const XT *X, int64_t ldx, const float *W,
                                       const float *b, int M, int K, int C, TileEnd &&tile_end) {
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, kg = lane >> 4;
    const int NC = (K + 63) / 64;         // double chunks per tile
    const int NH = half_chunks(K);        // half chunks of the image
    const int Cl = C - (NT - 1) * 16;     // classes of the last tile, 1..16
    const int cstride = chunk_bytes(NT, Cl);
    int *next = reinterpret_cast<int *>(lds + NH * cstride);
    if (threadIdx.x == 0) *next = 0;
    __syncthreads();
    const int n_tiles = (M + 15) >> 4;
    auto grab = [&]() -> int {  // the workgroup's next tile (block + grid * m), or -1
        int m = 0;
        if (lane == 0) m = atomicAdd(next, 1);
        m = __builtin_amdgcn_readfirstlane(m);
        const int t = (int)blockIdx.x + (int)gridDim.x * m;
        return t < n_tiles ? t : -1;
    };
    const auto xd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<XT *>(X), 0, (int)((int64_t)M * ldx * 2), 0x00020000);  // < 2^31, ldx even
    const uint32_t seg = 16u * (2 * kg + (j >> 3));
    const uint32_t pitch8 = (uint32_t)(8 * ldx * 2);
    int ltile = grab(), lc = 0;
    uint32_t lrow0 = 0, lrow1 = 0;
    auto rows_of = [&](int tile) {
        const int row = tile * 16 + (j & 7);
        lrow0 = (tile >= 0 && row < M) ? (uint32_t)((int64_t)row * ldx * 2) + seg : kOffOOB;
        lrow1 = (tile >= 0 && row + 8 < M) ? lrow0 + pitch8 : kOffOOB;
    };
    rows_of(ltile);
    constexpr int D = kDepth;
    u32x4 xa[D], xb[D];
    int stile[D], sc[D];
    auto load = [&](auto uc) {
        constexpr int u = decltype(uc)::value;
        stile[u] = ltile;
        sc[u] = lc;
        const uint32_t co = (uint32_t)lc * 128u;
        xa[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xd, lrow0 + co, 0, 0));
        xb[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xd, lrow1 + co, 0, 0));
        if (ltile >= 0 && ++lc == NC) {
            lc = 0;
            ltile = grab();
            rows_of(ltile);
        }
    };
    // the ring's first double chunks are in flight while W's image is built
    each_slot<0, D>(load);
    {
        // one unit = 8 k (a granule) of one class row, split into its three
        // pieces and stored at its lane's place in its half chunk's operand
        // block; units run in image order (half chunk, kg) along W's rows:
        // granule (hc, kg) is k = 64 (hc >> 1) + 16 kg + 8 (hc & 1)
        const auto wd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0,
                                                          (int)((int64_t)C * K * 4), 0x00020000);
        const int full = (NT - 1) * 64;
        const int G = NH * 4;  // granules per class row
        constexpr int FU = 8;  // units per thread per round, loads all issued first
        for (int base = threadIdx.x; base < C * G; base += FU * 64 * NW) {
            f32x4 e[FU][2];
            int dsto[FU];
#pragma unroll
            for (int f = 0; f < FU; ++f) {
                const int idx = base + f * 64 * NW;
                const bool in = idx < C * G;
                const int r = in ? idx / G : 0, g = in ? idx - r * G : 0;
                const int hc = g >> 2, kk = g & 3, n = r >> 4, jj = r & 15;
                const int k0 = 64 * (hc >> 1) + 16 * kk + 8 * (hc & 1);
                const int w = n < NT - 1 ? n * 64 + jj + 16 * kk : full + kk * Cl + jj;
                dsto[f] = in ? hc * cstride + w * 48 : -1;
                // (a granule wholly past K reads nothing: its offset may lie in the next row)
                const uint32_t off = k0 < K ? (uint32_t)(r * K + k0) * 4u : kOffOOB;
                e[f][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wd, off, 0, 0));
                e[f][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wd, off + 16, 0, 0));
                if (k0 + 8 > K) {  // the row's last granule: k >= K is the next row
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (k0 + q >= K) e[f][q >> 2][q & 3] = 0.0f;
                }
            }
#pragma unroll
            for (int f = 0; f < FU; ++f) {
                uint32_t h[4], m[4], l[4];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    split3(e[f][p >> 1][2 * (p & 1)], e[f][p >> 1][2 * (p & 1) + 1], h[p], m[p], l[p]);
                if (dsto[f] >= 0) {
                    char *dst = lds + dsto[f];
                    *reinterpret_cast<u32x4 *>(dst) = u32x4{h[0], h[1], h[2], h[3]};
                    *reinterpret_cast<u32x4 *>(dst + 16) = u32x4{m[0], m[1], m[2], m[3]};
                    *reinterpret_cast<u32x4 *>(dst + 32) = u32x4{l[0], l[1], l[2], l[3]};
                }
            }
        }
        // the zero granule of each half chunk's last class tile (its lanes past Cl)
        for (int c = threadIdx.x; c < NH; c += 64 * NW) {
            char *dst = lds + c * cstride + (full + 4 * Cl) * 48;
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x4 *>(dst + 16 * p) = u32x4{0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();
    // a lane's operand granules: full tile n at bfull + n * 3072, the last
    // tile at blast (the zero granule for lanes past its Cl classes); piece p
    // at + 16 p; half chunk hc at + hc * cstride
    const uint32_t bfull = (uint32_t)lane * 48u;
    const uint32_t blast = (NT - 1) * 3072u + 48u * (uint32_t)(j < Cl ? kg * Cl + j : 4 * Cl);
    f32x4 bias[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cl = n * 16 + 4 * kg + r;
            bias[n][r] = (b && cl < C) ? b[cl] : 0.0f;
        }
    f32x4 accH[NT], accL[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) accH[n] = accL[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool low = j < 8;
    auto step = [&](auto uc) -> bool {  // false: the stream is done (uniform)
        constexpr int u = decltype(uc)::value;
        const int tile = stile[u], c = sc[u];
        if (tile < 0) return false;
        const u32x4 A = xa[u], B = xb[u];
        uint32_t v[8];  // dword d: k = 64c + 16kg + 2d, + 1 of row j
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t t = ror8(low ? B[e] : A[e]);
            v[e] = low ? A[e] : t;
            v[4 + e] = low ? t : B[e];
        }
        load(uc);  // the double chunk D ahead into the slot just consumed
        if ((c + 1) * 64 > K) {  // the ragged last double chunk (uniform)
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int k = c * 64 + 16 * kg + 2 * d;
                v[d] = k >= K ? 0u : k + 1 >= K ? (v[d] & 0xffffu) : v[d];
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int hc = 2 * c + q;
            if (hc >= NH) continue;  // wholly past K (uniform): no image, no MFMAs
            u32x4 bw[NT][3];
            {
                const uint32_t coff = (uint32_t)hc * (uint32_t)cstride;
                const char *af = lds + bfull + coff;
                const char *al = lds + blast + coff;
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        bw[n][p] = *reinterpret_cast<const u32x4 *>(
                            (n < NT - 1 ? af + n * 3072 : al) + 16 * p);
            }
            uint32_t ah[4], am[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) pieces16<XT>(v[4 * q + p], ah[p], am[p]);
            const bf16x8_t Xh = __builtin_bit_cast(bf16x8_t, u32x4{ah[0], ah[1], ah[2], ah[3]});
            auto wb = [&](int n, int p) { return __builtin_bit_cast(bf16x8_t, bw[n][p]); };
#pragma unroll
            for (int n = 0; n < NT; ++n)
                accH[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 0), Xh, accH[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < NT; ++n)
                accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 1), Xh, accL[n], 0, 0, 0);
            if constexpr (__is_same(XT, f16_t)) {
                const bf16x8_t Xm = __builtin_bit_cast(bf16x8_t, u32x4{am[0], am[1], am[2], am[3]});
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 0), Xm, accL[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 2), Xh, accL[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 1), Xm, accL[n], 0, 0, 0);
            } else {
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    accL[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb(n, 2), Xh, accL[n], 0, 0, 0);
            }
        }
        if (c == NC - 1) {  // tile done: D[4 kg + r][j] = class n * 16 + 4 kg + r, row j
            f32x4 z[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                z[n] = accH[n] + accL[n] + bias[n];
                accH[n] = accL[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            tile_end(tile, z);
        }
        return true;
    };
    for (;;) {
        if (!run_slots<0, D>(step)) break;
    }
}

// ---------------------------------------------------------------------------
// Weight backward, modelled on xent_dw_cols_kernel (up to 48 classes): R row
// ranges x 64-column blocks, a wave takes every fourth 32-row step of its
// range, dY one 4/8/12-B load per row split in three, the next step's loads
// issued before the MFMAs, the waves' sums combined in LDS in wave order, the
// same partial layout (xent_reduce_dw_db_kernel is reused unchanged) and the
// same XCD numbering.  Per step lane (g, i) reads X rows 32s + 8g + t (t < 8),
// columns c0 + 4i .. c0 + 4i + 3: one 8-B load per row (4 rows x 128 B per
// instruction).  The B operand of N-tile e is rows 8g .. 8g + 7 of column
// c0 + 4i + e: one v_perm_b32 per dword (rows 2q, 2q + 1 of column e) and no
// split for bf16; fp16 widens the two halves and splits in two.
constexpr int kDw16Ranges = 48;  // row ranges (a multiple of 8: the XCD numbering)
constexpr int kDw16Width = 64;   // columns per block

// The grid of either form: column blocks x row ranges rounded up to the 8 XCDs.
inline int dw_cols_blocks(int K, int R, int *n_cblk) {
    *n_cblk = (K + kDw16Width - 1) / kDw16Width;
    return *n_cblk * ((R + 7) / 8) * 8;
}

template <int NT>
__device__ __forceinline__ void load_floats(__amdgpu_buffer_rsrc_t r, uint32_t off, float (&v)[NT]) {
    static_assert(NT >= 1 && NT <= 3, "1-3 floats");
    if constexpr (NT == 3) {
        typedef float f3 __attribute__((ext_vector_type(3)));
        const f3 x = __builtin_bit_cast(f3, __builtin_amdgcn_raw_buffer_load_b96(r, off, 0, 0));
        v[0] = x[0];
        v[1] = x[1];
        v[2] = x[2];
    } else if constexpr (NT == 2) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const f2 x = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
        v[0] = x[0];
        v[1] = x[1];
    } else {
        v[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
    }
}

template <int NT, typename XT>
__device__ __forceinline__ void dw_cols(const XT *X, int64_t ldx, const float *G, int ldg, int M,
                                        int K, int C, int n_cblk, int R, float *slab,
                                        float *db_slab) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    constexpr bool kF16 = __is_same(XT, f16_t);
    constexpr int XP = kF16 ? 2 : 1;  // pieces of x
    __shared__ f32x4 red[4][NT][4][64];  // [wave][class tile][q][lane] -> N-tiles e = 0..3
    __shared__ float dbr[4][NT * 16];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform loop bounds
    const int i = lane & 15, g = lane >> 4;
    const int q8 = (int)blockIdx.x >> 3;
    const int cb = q8 % n_cblk, r = (q8 / n_cblk) * 8 + ((int)blockIdx.x & 7);
    if (r >= R) return;  // (uniform per block: no barrier reached)
    const int S = (M + 31) >> 5;
    const int c0 = cb * kDw16Width;
    const int Ke = (K + 1) & ~1;  // a step's range ends on a dword (ldx is even and >= K)
    const uint32_t xpitch = (uint32_t)ldx * 2u, gpitch = (uint32_t)ldg * 4u;
    // a lane whose four columns all lie past K reads nothing
    const uint32_t xlane = c0 + 4 * i < K ? (uint32_t)(8 * g * ldx + c0 + 4 * i) * 2u : kOffOOB;
    // classes NT i + n; a lane whose first class is past C reads nothing
    const uint32_t glane = NT * i < C ? (uint32_t)(8 * g * ldg + NT * i) * 4u : kOffOOB;
    u32x2 xr[8];
    float gr[8][NT];
    const int w_a = w, w_b = (S - r + R - 1) / R, w_step = 4;
    auto load = [&](int j) {
        const int s = r + R * j;
        const int rows = s < S ? min(32, M - 32 * s) : 0;
        const int64_t row0 = s < S ? 32 * (int64_t)s : 0;
        const auto xd = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<XT *>(X + row0 * ldx), 0, rows ? (int)(((int64_t)(rows - 1) * ldx + Ke) * 2) : 0,
            0x00020000);
        const auto gd = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float *>(G + row0 * ldg), 0, rows ? (int)(((int64_t)(rows - 1) * ldg + C) * 4) : 0,
            0x00020000);
        // (the lane offsets opaque per step, as in xent_dw_cols_kernel)
        uint32_t xl = xlane, gl = glane;
        asm volatile("" : "+v"(xl), "+v"(gl));
#pragma unroll
        for (int t = 0; t < 8; ++t)
            xr[t] = __builtin_bit_cast(
                u32x2, __builtin_amdgcn_raw_buffer_load_b64(xd, xl + (uint32_t)t * xpitch, 0, 0));
#pragma unroll
        for (int t = 0; t < 8; ++t) load_floats<NT>(gd, gl + (uint32_t)t * gpitch, gr[t]);
    };
    // hh products in accH, the small ones in accL (as the forward)
    f32x4 accH[NT][4], accL[NT][4];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            accH[n][e] = f32x4{0.f, 0.f, 0.f, 0.f};
            accL[n][e] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    const bool sum_db = db_slab && cb == 0;  // column block 0 also sums dY's rows
    float dba[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dba[n] = 0.f;
    load(w_a);
    for (int st = w_a; st < w_b; st += w_step) {
        u32x4 ga[NT][3], xb[4][XP];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t h, m, lo;
                split3(gr[2 * q][n], gr[2 * q + 1][n], h, m, lo);
                ga[n][0][q] = h;
                ga[n][1][q] = m;
                ga[n][2][q] = lo;
            }
        if (sum_db) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int t = 0; t < 8; ++t) dba[n] += gr[t][n];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // rows 2q (low half) and 2q + 1 of column e: bytes 0-3 of the
                // selector index the second operand, 4-7 the first
                const uint32_t pr = __builtin_amdgcn_perm(xr[2 * q + 1][e >> 1], xr[2 * q][e >> 1],
                                                          (e & 1) ? 0x07060302u : 0x05040100u);
                uint32_t h, m;
                pieces16<XT>(pr, h, m);
                xb[e][0][q] = h;
                if constexpr (kF16) xb[e][1][q] = m;
            }
        load(st + w_step);
        // the next step's loads go out before this step's MFMAs
        __builtin_amdgcn_sched_barrier(0);
        auto A = [&](int n, int p) { return __builtin_bit_cast(bf16x8_t, ga[n][p]); };
        auto B = [&](int e, int p) { return __builtin_bit_cast(bf16x8_t, xb[e][p]); };
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                accH[n][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A(n, 0), B(e, 0), accH[n][e], 0, 0, 0);
                accL[n][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A(n, 1), B(e, 0), accL[n][e], 0, 0, 0);
                if constexpr (kF16)
                    accL[n][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A(n, 0), B(e, 1), accL[n][e], 0, 0, 0);
                accL[n][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A(n, 2), B(e, 0), accL[n][e], 0, 0, 0);
                if constexpr (kF16)
                    accL[n][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A(n, 1), B(e, 1), accL[n][e], 0, 0, 0);
            }
    }
    // D[row 4g + q][j = i] of tile (n, e) -> class NT (4g + q) + n, column c0 + 4i + e
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            red[w][n][q][lane] = f32x4{accH[n][0][q] + accL[n][0][q], accH[n][1][q] + accL[n][1][q],
                                       accH[n][2][q] + accL[n][2][q], accH[n][3][q] + accL[n][3][q]};
    if (sum_db) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            float v = dba[n];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (g == 0) dbr[w][NT * i + n] = v;
        }
    }
    __syncthreads();
    // the block's partial: classes < C x its columns < K, the waves in order
    const int col = threadIdx.x & 63;
    const float *rf = reinterpret_cast<const float *>(red);
    float *out = slab + (int64_t)r * (NT * 16) * K;
    if (c0 + col < K) {
        for (int cls = threadIdx.x >> 6; cls < C; cls += 4) {
            const int r4 = cls / NT, n = cls - r4 * NT, gg = r4 >> 2, q = r4 & 3;
            const int at = ((n * 4 + q) * 64) * 4 + 64 * gg + col;
            constexpr int wstride = NT * 4 * 64 * 4;
            out[(int64_t)cls * K + c0 + col] =
                ((rf[at] + rf[at + wstride]) + rf[at + 2 * wstride]) + rf[at + 3 * wstride];
        }
    }
    if (sum_db && (int)threadIdx.x < C)
        db_slab[(int64_t)r * (NT * 16) + threadIdx.x] =
            ((dbr[0][threadIdx.x] + dbr[1][threadIdx.x]) + dbr[2][threadIdx.x]) + dbr[3][threadIdx.x];
}

}  // namespace x16
}  // namespace sgc
