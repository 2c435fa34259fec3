/*
 * sgc_amd.h -- C ABI of libsgc_amd.so, the MI355X (gfx950) propagation engine
 * behind SGC's sgc_precompute() / SGC.forward().
 *
 * The reference (bellaj09/SGC) has no native code and no FFI: its hot path is
 * three lines of Python calling torch (utils.py:92-97 -> torch.spmm at
 * utils.py:95; models.py:17-18 -> nn.Linear).  Each entry point below names
 * the reference call it replaces.  Conventions:
 *
 *   - every pointer is a DEVICE pointer unless the parameter name ends in
 *     _host; buffers are owned by the caller (torch), never freed here;
 *   - `stream` is a hipStream_t passed as void* (torch:
 *     torch.cuda.current_stream().cuda_stream); all work is enqueued
 *     asynchronously on it; nothing here synchronises the device except the
 *     calls documented as "synchronous";
 *   - return 0 on success, a positive SGC_E* code on failure;
 *     sgc_last_error() returns a thread-local message for the last failure;
 *   - thread safety: every entry point may be called from several host
 *     threads at once (on different streams); the SpMM's internal side
 *     stream (hub rows) is serialised per device so one call's fork/join
 *     never interleaves with another's;
 *   - indices are int32 (n_rows, n_cols, nnz < 2^31), values fp32.
 */
#ifndef SGC_AMD_H
#define SGC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGC_ABI_VERSION 1

enum {
    SGC_OK = 0,
    SGC_EINVAL = 1,   /* bad argument (shape, stride, alignment, null)   */
    SGC_ERANGE = 2,   /* size or index outside the int32 CSR limits      */
    SGC_EHIP = 3,     /* a HIP runtime call failed                       */
    SGC_ENOMEM = 4,   /* workspace too small                             */
    SGC_EDEVICE = 5   /* no gfx950 device / kernel image not loadable    */
};

int sgc_abi_version(void);
const char *sgc_last_error(void);

/* Process-wide schedule knobs (results never depend on them).
 *   "slice_floats": feature-slice width of the SpMM grid in floats (default
 *                   128 = one 64V-float chunk per slice; 0 = one slice as wide
 *                   as the registers allow);
 *   "max_vec":      widest per-lane load, 1, 2 or 4 floats (default 4);
 *   "hub_chunk":    features per hub-kernel workgroup, 32 or 64 (default 0 =
 *                   32 when F <= 192 and X rows are 128-B aligned, else 64);
 *   "hub_stream":   1 = hub kernel on a side stream, concurrent with the
 *                   light kernel; 2 = on the caller's stream before the light
 *                   kernel (serial, no cross-stream events); 0 = default: the
 *                   side stream unless the launch sets SGC_SPMM_HUB_SERIAL;
 *   "rows_per_wave": light rows per wavefront when 16-B lanes are possible
 *                   (0 = default, auto; 2 = 32 lanes x 4 floats per row; 4 =
 *                   16 lanes; 1 = one row per wave with the slice_floats /
 *                   max_vec scheme);
 *   "hub_loaders":  loader waves per hub workgroup, 15 (default) or 7;
 *   "hub_fuse":     1 (default) = serial hub rows (SGC_SPMM_HUB_SERIAL) run as
 *                   the first workgroups of the light kernel's own launch
 *                   (three loader waves + the chain wave each) where that is
 *                   the multi-row kernel over 16-B-lane slices or the
 *                   one-chunk csr kernel; 0 = their own launch before it;
 *   "heavy_pairs":  heavy-row load forms, a bit mask (default 29): 1 pairs in
 *                   the multi-row kernel, 2 in the one-row kernel, 4 four
 *                   nonzeros per load up to 32 floats, 8 the same transposed
 *                   at 33..64 floats, 16 the pairs transposed;
 *   "x16_vec":      widest per-lane load of the 16-bit-feature launches, 8,
 *                   4, 2 or 1 elements (feature slices of 64 x that); 0 =
 *                   default: 8 up to 512 features (one slice), else 4;
 *   "x16_step":     nonzeros per step of their light rows at 16-B lanes, 8
 *                   or 4 (two steps in flight); 0 = default: 4 on launches
 *                   below 65,536 rows, else 8;
 *   "tile_buffers": classifier LDS tile images, 1 (default) or 2;
 *   "linear_kernel": classifier forward, 0 = auto (the streaming kernel where
 *                   W^T fits LDS and M >= 4096), 1 = LDS tile, 2 = streaming
 *                   (3 / 4: its diagnostic forms -- loads only / MFMAs only --
 *                   whose results are wrong by design);
 *   "linear_ck":    k per chunk of the streaming forward, 64 (default) or 32;
 *   "backward_kernel": classifier weight backward, 0 = auto (split-bf16
 *                   column blocks up to 48 classes, else the fp32 MFMA
 *                   slabs), 1 = fp32 MFMA slabs, 2 = split-bf16 slabs where X
 *                   gives 8-B lanes (K and ldx even), 3 = split-bf16 column
 *                   blocks (up to 48 classes; more: as 0).  The split-bf16
 *                   kernels need finite X and dY: a non-finite x gives NaN
 *                   in its column of dW.  torch's non-finite semantics need
 *                   the fp32 kernels on both sides: "linear_kernel" = 2 AND
 *                   "backward_kernel" = 1;
 *   "short_wide":   wide items of the multi-row SpMM kernel: a light row of at
 *                   most Ts nonzeros crosses every feature slice in one wave
 *                   instead of one wave per slice (sgc_spmm_csr_f32_ex3).  -1
 *                   (default) = the rule: Ts = 16 on launches of at least
 *                   65,536 rows; 0 = off; 1..32 forces Ts on every launch that
 *                   can take wide items (32 lanes per row, a light order, at
 *                   least two slices, no fused hub rows).  Read-only beside
 *                   it: "short_wide_ts" = the Ts in force (0 = off), which a
 *                   caller of sgc_spmm_csr_f32_ex3 counts rows against, and
 *                   "short_wide_launches" = launches that took wide items,
 *                   "short_wide_state" = (knob + 1) * 64 + Ts in one read;
 *   "short_wide_first": 1 = the wide waves' workgroups come first in the
 *                   grid, 0 (default) = last;
 *   "adam_kernel":  schedule of sgc_train_adam_f32, 0 = auto (the small
 *                   schedule where it measured faster: M <= 313 and
 *                   16 M < K + 832), 1 = general, 2 = small (a
 *                   shape it cannot take runs the general one).  Read-only
 *                   beside it: "adam_kernel_last" = the schedule the last
 *                   call ran (1 / 2; 0 before the first) and
 *                   "adam_small_max_rows" = the small schedule's row limit,
 *                   "adam_sweep_last" = what the last
 *                   sgc_train_adam_sweep_f32 call ran (2 batched small, 1
 *                   general per model, 0 none yet);
 *   "adam_sweep_form": the second launch of sgc_train_adam_sweep_f32's batched
 *                   small schedule, 0 = rule (split where the fused form would
 *                   re-read at least 100 MB of partial logits per epoch),
 *                   1 = fused (one launch), 2 = split (two launches); the same
 *                   bits either way.  Read-only beside it:
 *                   "adam_sweep_form_last" (1 / 2; 0 before the first).
 * sgc_get_tuning returns -1 for an unknown key. */
int sgc_set_tuning(const char *key, int64_t value);
int64_t sgc_get_tuning(const char *key);

/* ---------------------------------------------------------------------------
 * Ingest: torch sparse COO -> CSR.
 * Replaces the implicit COO handling inside torch.spmm (utils.py:95) for the
 * adjacency built by sparse_mx_to_torch_sparse_tensor (utils.py:23-30:
 * int64 [2,nnz] indices, fp32 values).  The CSR keeps every stored entry
 * (no coalescing) and, within a row, the COO storage order (stable by row),
 * which is the order torch's CPU kernel applies its FMAs in.
 *
 * sgc_coo_to_csr_workspace: bytes of device scratch sgc_coo_to_csr needs.
 * sgc_coo_to_csr: rows/cols are the two rows of the [2,nnz] index tensor.
 *   status_host (may be NULL: the call is synchronous either way, it reads
 *   its flags back to choose the sorted or the unsorted path and to return
 *   SGC_ERANGE) receives a bit set: 1 = input rows already sorted, 2 = every
 *   CSR row has strictly ascending columns (of the CSR written, whether or
 *   not the input rows were sorted), 4 = an index was out of range (CSR then
 *   invalid).
 * ------------------------------------------------------------------------- */
int sgc_coo_to_csr_workspace(int64_t n_rows, int64_t nnz, size_t *bytes_host);
int sgc_coo_to_csr(const int64_t *rows, const int64_t *cols, const float *vals,
                   int64_t nnz, int64_t n_rows, int64_t n_cols,
                   int32_t *row_ptr, int32_t *col_idx, float *val_out,
                   void *workspace, size_t workspace_bytes,
                   uint32_t *status_host, void *stream);

/* Same, from torch CSR (crow_indices/col_indices int64): narrows to int32.
 * Status bit 1 is always set, bit 2 as above.  SGC_ERANGE with bit 4 for a
 * column outside [0, n_cols) and for a crow that is no layout of the nnz
 * entries: an element outside [0, nnz], a decrease, crow[0] != 0 or
 * crow[n_rows] != nnz. */
int sgc_csr64_to_csr(const int64_t *crow, const int64_t *col, const float *vals,
                     int64_t nnz, int64_t n_rows, int64_t n_cols,
                     int32_t *row_ptr, int32_t *col_idx, float *val_out,
                     uint32_t *status_host, void *stream);

/* ---------------------------------------------------------------------------
 * On-device augmented normalisation S = D^-1/2 (A+I) D^-1/2 (reference
 * normalization.py:5-12 + the fp32 rounding of utils.py:25): scipy's entries
 * and, where its value is not NaN, its fp32 bits (NaN where it is NaN; payload
 * and sign unspecified).  A: canonical CSR (ascending unique columns per row),
 * fp64 values.  Two passes around one host step, exactly as the reference
 * splits its arithmetic:
 *   1. sgc_augnorm_count: per-row entry count of A+I (exact zeros pruned: a
 *      stored +-0.0 of A, a_ii + 1 == 0) -> out_row_ptr (scan) and rowsum
 *      (fp64, sequential in column order); *out_nnz_host = nnz(A+I).
 *      Synchronous.  Returns SGC_EINVAL if A is not canonical.
 *   2. host: d = rowsum ** -0.5, inf -> 0 (numpy, as normalization.py:8-10);
 *      d is 0 for a sum of 0 or +-inf, NaN for a negative or NaN sum;
 *   3. sgc_augnorm_fill: S entries (d_i * a_ij) * d_j in fp64 -> fp32, in
 *      ascending column order.  An entry is dropped, as scipy's
 *      diags(d) . (A+I) . diags(d) drops it, when d_i == 0, d_j == 0,
 *      d_i * a_ij == 0 or the product == 0 -- decided in fp64, so 0 * inf and
 *      0 * NaN leave no entry while a product that only rounds to 0.0f stays
 *      one (out_row_ptr may shrink then; *out_nnz_host = final nnz).
 *      Synchronous.
 * workspace: sgc_augnorm_workspace(n) bytes of device scratch.
 * ------------------------------------------------------------------------- */
int64_t sgc_augnorm_workspace(int64_t n_rows);
int sgc_augnorm_count(const int32_t *row_ptr, const int32_t *col_idx, const double *val,
                      int64_t n_rows, int64_t nnz, int32_t *out_row_ptr, double *rowsum,
                      void *workspace, int64_t workspace_bytes, int64_t *out_nnz_host,
                      uint32_t *status_host, void *stream);
int sgc_augnorm_fill(const int32_t *row_ptr, const int32_t *col_idx, const double *val,
                     int64_t n_rows, const double *d, int32_t *out_row_ptr,
                     int32_t *out_col_idx, float *out_val, void *workspace,
                     int64_t workspace_bytes, int64_t *out_nnz_host, void *stream);

/* ---------------------------------------------------------------------------
 * Induced sub-graph B = A[idx][:, idx] (reference utils.py:117, the inductive
 * train sub-graph of reddit.py:44-47, taken on A + A^T before normalisation).
 * A: CSR (int32), fp64 values; idx: int64 [m], distinct ids in [0, n_rows).
 * B: canonical CSR (new row i = old row idx[i], new column = position in
 * idx, ascending), fp64 values -- the input sgc_augnorm_count/fill take, so
 * the S_train built from B is the reference's (as above).  Two synchronous
 * calls around the host allocation of B, sharing one workspace:
 *   sgc_subgraph_count: out_row_ptr [m+1], *out_nnz_host = nnz(B);
 *     status_host bits: 1 = repeated ids (SGC_EINVAL), 2 = idx ascending,
 *     4 = an id out of range (SGC_ERANGE);
 *   sgc_subgraph_fill: out_col_idx / out_val [nnz(B)].
 * workspace: sgc_subgraph_workspace(n_rows, m, nnz(A)) bytes.
 * ------------------------------------------------------------------------- */
int64_t sgc_subgraph_workspace(int64_t n_rows, int64_t m, int64_t nnz);
int sgc_subgraph_count(const int32_t *row_ptr, const int32_t *col_idx, int64_t n_rows,
                       int64_t nnz, const int64_t *idx, int64_t m, int32_t *out_row_ptr,
                       void *workspace, int64_t workspace_bytes, int64_t *out_nnz_host,
                       uint32_t *status_host, void *stream);
int sgc_subgraph_fill(const int32_t *row_ptr, const int32_t *col_idx, const double *val,
                      int64_t n_rows, int64_t nnz, const int64_t *idx, int64_t m,
                      const int32_t *out_row_ptr, int32_t *out_col_idx, double *out_val,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* CSR -> torch COO indices: rows64[k], cols64[k] (int64) of every entry. */
int sgc_csr_to_coo64(const int32_t *row_ptr, const int32_t *col_idx, int64_t n_rows,
                     int64_t *rows64, int64_t *cols64, void *stream);

/* ---------------------------------------------------------------------------
 * Schedule ("plan") for the SpMM.  Lists the rows of [row_begin, row_end)
 * with more than heavy_threshold nonzeros, heaviest first; the first n_hub
 * of them have more than hub_threshold (>= heavy_threshold).
 * sgc_spmm_csr_f32 runs
 *   - each hub row on 1024-thread workgroups (one per 64-feature chunk; 15
 *     waves gather nonzeros ahead into LDS, one runs the FMA chain), on a
 *     side stream joined back to the caller's stream;
 *   - each other heavy row as one wave per 128-float chunk, scheduled first;
 *   - every remaining row as one wave.
 * The plan changes only the schedule: every output element is still one
 * sequential FMA chain, so results never depend on it.  Synchronous (reads
 * the heavy-row list back to sort it).
 *
 * plan must hold sgc_plan_capacity(row_end - row_begin) int32 words;
 * *n_heavy_host receives the number of heavy rows written to plan[0..),
 * *n_hub_host (may be NULL) how many of them lead as hub rows.
 * ------------------------------------------------------------------------- */
int64_t sgc_plan_capacity(int64_t n_rows);
int sgc_plan_build(const int32_t *row_ptr, int64_t row_begin, int64_t row_end,
                   int32_t heavy_threshold, int32_t hub_threshold, int32_t *plan,
                   int64_t plan_capacity, int64_t *n_heavy_host, int64_t *n_hub_host,
                   void *stream);
/* The light rows' processing order for SGC_SPMM_LIGHT_ORDER: every row of
 * [row_begin, row_end) with at most heavy_threshold nonzeros, longest first,
 * ties in row order (a stable counting sort on the host after one read-back
 * of row_ptr), written to light[0 .. *n_light_host) on the device (light
 * must hold row_end - row_begin words); synchronous on `stream`.  Place it
 * after the n_heavy rows of sgc_plan_build's plan.  A schedule only. */
int sgc_plan_light_order(const int32_t *row_ptr, int64_t row_begin, int64_t row_end,
                         int32_t heavy_threshold, int32_t *light, int64_t *n_light_host,
                         void *stream);

/* ---------------------------------------------------------------------------
 * One hop Y = S[row_begin:row_end, :] . X  (utils.py:95, torch.spmm).
 * Y row 0 receives S row row_begin.  Each Y[i,f] is
 *     acc = +0.0f; for k in row i (CSR order): acc = fmaf(val[k], X[col[k], f], acc)
 * -- bit-identical to the reference CPU kernel.  X rows have stride ldx
 * floats, Y rows ldy floats; X must not alias Y.
 * Special values (IEEE 754 binary32, no flush to zero, on every schedule):
 * Y[i,f] is NaN exactly where the reference's result is NaN; the payload and
 * the sign of a NaN are unspecified.  Every other element is bit-equal,
 * signed zeros (a chain whose products all underflow to -0 ends in -0.0; an
 * empty row gives +0.0), subnormal operands and results, and overflow to
 * +-inf included.  No FMA is issued beyond the row's stored entries: a pad
 * lane or a re-read last nonzero never reaches a chain.
 * plan/n_heavy/n_hub/heavy_threshold from sgc_plan_build over the same row
 * range, or plan = NULL (one work item per row, natural order).
 * ------------------------------------------------------------------------- */
int sgc_spmm_csr_f32(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                     int64_t row_begin, int64_t row_end,
                     const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                     const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                     int32_t heavy_threshold, void *stream);

/* Per-kernel launch timing (diagnostics; off by default).  While enabled,
 * every sgc_spmm_csr_f32 records timing events around its light/heavy-row
 * kernel and around its hub-row kernel, each on the stream that kernel runs
 * on.  sgc_timing_collect waits for the recorded launches (synchronous) and
 * writes, in launch order, light_ms_host[i] and hub_ms_host[i] (-1 when the
 * launch had no hub rows); *n_host = launches recorded since the last
 * collect (SGC_ENOMEM when capacity is smaller; nothing is consumed then).
 * Do not enable while capturing a graph. */
int sgc_timing_enable(int on);
int sgc_timing_collect(float *light_ms_host, float *hub_ms_host, int64_t capacity,
                       int64_t *n_host);
/* Same, plus per launch: span_ms_host[i] = the whole launch (first kernel
 * start to the later kernel end: what the caller's stream waits for) and
 * light_kernel_host[i] = which light/heavy-row kernel ran (0 spmm_csr_kernel,
 * 1 spmm_rows_kernel, 2 / 3 spmm_rows_kernel / spmm_csr_kernel with the
 * serial hub rows fused into its launch, -1 none: a hub-only launch).  Either
 * may be NULL. */
int sgc_timing_collect_ex(float *light_ms_host, float *hub_ms_host, float *span_ms_host,
                          int32_t *light_kernel_host, int64_t capacity, int64_t *n_host);

/* Same, with flags.
 * Layout, for buffers whose rows are padded (the engine's own 128-B-row
 * buffers): SGC_SPMM_X_PADDED = X's columns [F, round4(F)) are allocated in
 * every row and may be read (their values do not matter); SGC_SPMM_Y_PADDED
 * = Y's columns [F, round4(F)) are allocated and may be overwritten with
 * don't-care values.  They let the kernel use 16-B lanes at any F; columns
 * < F are bit-identical either way.
 * Split launch of one hop (the multi-GPU pipeline runs the hub rows beside
 * several narrower launches): SGC_SPMM_NO_HUB = skip the plan's n_hub hub
 * rows (their Y rows are not written); SGC_SPMM_HUB_ONLY = only the hub rows,
 * on `stream` itself (no side stream).  The two launches together write
 * exactly what one unflagged launch writes.
 * Column-block passes (the multi-GPU pipeline that consumes an exchange in
 * column order, sgc_amd.distributed.CyclicRowPropagator): SGC_SPMM_ACCUMULATE
 * = each element's FMA chain starts from Y's current value instead of +0.0f,
 * and rows without nonzeros in this CSR are left untouched.  When S's
 * nonzeros are split by column range into CSRs S_0, S_1, ... (each row's
 * nonzeros of S_g precede those of S_{g+1} in CSR order), one unflagged
 * launch over S_0 followed by ACCUMULATE launches over S_1, S_2, ... writes
 * exactly what one launch over S writes (the fp32 store/load between passes
 * is exact).
 * SGC_SPMM_HUB_SERIAL: run the hub rows' kernel on `stream` before the light
 * kernel instead of beside it on a side stream (no fork/join events); for
 * launches whose longest hub chain is shorter than the ~20-30 us a
 * cross-stream fork/join costs (sgc_set_tuning "hub_stream" overrides).
 * SGC_SPMM_LIGHT_ORDER: `plan` holds row_end - row_begin entries: its n_heavy
 * heavy rows (as sgc_plan_build writes them) followed by every other row of
 * the range, in the order the light rows are to be processed (the Python
 * layer sorts them by length, so the rows sharing a wavefront in the
 * multi-row kernel have about the same length and few lanes idle-load past
 * their row's end).  A schedule only: results never depend on it.
 * SGC_SPMM_X_UNDER_4G: the caller vouches that X has fewer than 2^24 rows
 * and that every X row a column id can name lies within 4 GiB of X
 * (n_cols * ldx * 4 < 2^32), so the gathers may use 32-bit row offsets from
 * one 24-bit multiply (fewer address instructions per nonzero).  The library
 * cannot check it (it never sees n_cols here): a caller that sets the flag
 * for a larger X gets wrapped addresses -- wrong rows gathered -- not an
 * error.  sgc_propagate_f32 / sgc_propagate_groups_f32 and the Python layer
 * derive it themselves from n_rows and the row stride.  */
enum { SGC_SPMM_X_PADDED = 1, SGC_SPMM_Y_PADDED = 2, SGC_SPMM_NO_HUB = 4,
       SGC_SPMM_HUB_ONLY = 8, SGC_SPMM_ACCUMULATE = 16, SGC_SPMM_HUB_SERIAL = 32,
       SGC_SPMM_LIGHT_ORDER = 64, SGC_SPMM_X_UNDER_4G = 128 };
int sgc_spmm_csr_f32_ex(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                        int64_t row_begin, int64_t row_end,
                        const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                        const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                        int32_t heavy_threshold, uint32_t flags, void *stream);

/* sgc_spmm_csr_f32_ex with the plan's count of rows that have at least one
 * nonzero (n_nonempty = counts_host[3] of sgc_plan_sorted_ex; < 0 = unknown,
 * which is sgc_spmm_csr_f32_ex).  It matters to SGC_SPMM_ACCUMULATE launches
 * with SGC_SPMM_LIGHT_ORDER: they leave rows without nonzeros untouched, the
 * plan lists those rows last, so the multi-row kernel's light items stop at
 * n_nonempty - n_heavy and no wave is started for an empty row (the one-row
 * kernel keeps its row order over all rows: measured faster there; a column
 * group's accumulate pass at Reddit shape: 12 % of the rows in the pure split,
 * 73 % with whole rows of <= 32 nonzeros, sgc_csr_colsplit_ex).  Plain
 * launches cover every row as before (an empty row is written as zeros).
 * A schedule only: the results are those of sgc_spmm_csr_f32_ex. */
int sgc_spmm_csr_f32_ex2(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                         int64_t row_begin, int64_t row_end,
                         const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                         const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                         int32_t heavy_threshold, uint32_t flags, int64_t n_nonempty,
                         void *stream);

/* sgc_spmm_csr_f32_ex2 with wide items: n_not_wide = the plan's light rows
 * (rows of at most heavy_threshold nonzeros) with MORE than wide_max_nnz
 * nonzeros, wide_max_nnz = sgc_get_tuning("short_wide_ts") in 1..32
 * (sgc_plan_sorted_ex2 counts the rows above 4 / 8 / 16 / 32: n_not_wide =
 * that count - n_heavy).  With SGC_SPMM_LIGHT_ORDER the sorted plan lists
 * those rows first among the light ones; the light rows after them -- up to
 * n_nonempty in an SGC_SPMM_ACCUMULATE launch, else to the end, the rows
 * without nonzeros included (written as zeros) -- run as wide items where the
 * "short_wide" knob and the launch allow: one wave carries two such rows
 * through every feature slice and no per-slice wave is started for them.
 * n_not_wide < 0 is sgc_spmm_csr_f32_ex2 exactly.  A schedule only: every
 * (row, feature) FMA chain is unchanged, so are the results; a count that
 * does not match the plan gives wrong values for the miscounted rows. */
int sgc_spmm_csr_f32_ex3(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                         int64_t row_begin, int64_t row_end,
                         const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                         const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                         int32_t heavy_threshold, uint32_t flags, int64_t n_nonempty,
                         int64_t n_not_wide, int32_t wide_max_nnz, void *stream);

/* Which kernels an sgc_spmm_csr_f32_ex3 launch of these arguments would run
 * under the knobs in force (measurement and tests; the counterpart of
 * sgc_linear_kernel_name).  Host only: it needs no device, X and Y are used
 * for their alignment and never dereferenced, plan for being NULL or not.
 * Returns a thread-local string, valid until the thread's next call:
 *   "spmm_rows_kernel<LB=..,VH=..,UH=16,O32=..,QV=..,HF=..,WD=..> LR=.. slices=..
 *    n_sub=.. bits=<heavy_pairs / pipe2 bits passed> grid=XxY wide=<wide items>
 *    hub=<none|concurrent|serial|fused>[ spmm_hub_kernel<HC,NL> grid=..]"
 * or "spmm_csr_kernel<V=..,C=..,UH=16,HF=..> LR=0 slices=.. n_sub=.. bits=.. grid=XxY
 *    wide=0 hub=..";
 * "none" for a launch that runs no light kernel (no rows, SGC_SPMM_HUB_ONLY)
 * and for arguments sgc_spmm_csr_f32_ex3 would reject (sgc_last_error says why). */
const char *sgc_spmm_kernel_name(int64_t row_begin, int64_t row_end, const float *X, int64_t ldx,
                                 const float *Y, int64_t ldy, int64_t F, const int32_t *plan,
                                 int64_t n_heavy, int64_t n_hub, int32_t heavy_threshold,
                                 uint32_t flags, int64_t n_nonempty, int64_t n_not_wide,
                                 int32_t wide_max_nnz);

/* K hops X_K = S^K X_0 over all n_rows rows (utils.py:92-97, the whole
 * sgc_precompute loop).  out (row stride ldo) receives X_K.  Intermediate
 * hops live in the workspace with 128-B aligned rows (ld = F rounded up to 32
 * floats: a gathered X row segment then spans the fewest 128-B lines); when
 * X_0's rows are not 128-B aligned it is first copied into that layout
 * (sgc_pad_rows_f32), which costs one streaming copy and saves ~9% per hop
 * that reads it at Reddit shape.  K = 0 copies X_0 into out (the Python
 * layer returns the input object itself, as the reference does).
 * sgc_propagate_workspace: bytes of device workspace for these arguments. */
int64_t sgc_propagate_workspace(int64_t n_rows, int64_t F, int64_t ldx, int32_t K);
int sgc_propagate_f32(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                      int64_t n_rows, const float *X0, int64_t ldx, float *out,
                      int64_t ldo, int64_t F, int32_t K,
                      const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                      int32_t heavy_threshold, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* The same loop over S split into `groups` column groups (sgc_csr_colsplit:
 * row_ptrs [groups][n_rows+1] absolute into one col_idx / val pair; rows with
 * ascending columns), each hop as `groups` launches -- group 0 plain, groups
 * 1.. with SGC_SPMM_ACCUMULATE -- which is bit-identical to one launch per
 * hop and faster at Reddit shape.  Per group g:
 * plans_host[g] / n_heavy_host[g] / n_hub_host[g] / thresholds_host[g] =
 * sgc_plan_sorted over group g's CSR (plans_host NULL = no plans), and
 * plan_flags_host[g] (may be NULL) = SGC_SPMM_LIGHT_ORDER (plans_host[g]
 * lists every row, as sgc_plan_sorted writes it) | SGC_SPMM_HUB_SERIAL.
 * groups = 1 with row_ptrs = the CSR's row_ptr is sgc_propagate_f32 with
 * plan flags.  Same workspace as sgc_propagate_f32. */
int sgc_propagate_groups_f32(int32_t groups, const int32_t *row_ptrs, const int32_t *col_idx,
                             const float *val, int64_t n_rows, const float *X0, int64_t ldx,
                             float *out, int64_t ldo, int64_t F, int32_t K,
                             const int32_t *const *plans_host, const int64_t *n_heavy_host,
                             const int64_t *n_hub_host, const int32_t *thresholds_host,
                             const uint32_t *plan_flags_host, void *workspace,
                             int64_t workspace_bytes, void *stream);
/* The same with, per group, the plan's rows with nonzeros (n_nonempty_host,
 * sgc_spmm_csr_f32_ex2) and its light rows above wide_max_nnz nonzeros
 * (n_not_wide_host, sgc_spmm_csr_f32_ex3); either may be NULL (= unknown). */
int sgc_propagate_groups_f32_ex3(int32_t groups, const int32_t *row_ptrs, const int32_t *col_idx,
                                 const float *val, int64_t n_rows, const float *X0, int64_t ldx,
                                 float *out, int64_t ldo, int64_t F, int32_t K,
                                 const int32_t *const *plans_host, const int64_t *n_heavy_host,
                                 const int64_t *n_hub_host, const int32_t *thresholds_host,
                                 const uint32_t *plan_flags_host,
                                 const int64_t *n_nonempty_host, const int64_t *n_not_wide_host,
                                 int32_t wide_max_nnz, void *workspace, int64_t workspace_bytes,
                                 void *stream);

/* Row-strided copy dst[i, 0:F] = src[i, 0:F] (re-layout of feature rows). */
int sgc_pad_rows_f32(const float *src, int64_t lds, float *dst, int64_t ldd,
                     int64_t n_rows, int64_t F, void *stream);

/* Batched 2-D block copy, one launch (the multi-GPU exchanges' unpack,
 * sgc_amd.distributed): for each of nseg <= 64 segments, segs_host[6s ..
 * 6s+5] = (src_row, src_col, dst_row, dst_col, rows, cols):
 *     dst[dst_row + i, dst_col + j] = src[src_row + i, src_col + j],
 * i < rows, j < cols; row strides lds / ldd (floats).  Segments must not
 * overlap in dst.  Replaces the P strided copies that landed each rank's
 * column block of an all-gathered row chunk in X_K (the reference returns the
 * whole X_K from utils.py:92-97, so every rank needs all of it). */
int sgc_copy_blocks_f32(const float *src, int64_t lds, float *dst, int64_t ldd, int32_t nseg,
                        const int64_t *segs_host, void *stream);

/* Peer exchange over IPC-mapped memory: the replicated output of the
 * partitioned sgc_precompute (utils.py:92-97 returns all of X_K to every
 * caller) without a gathered copy.  Each rank exposes one buffer of its own
 * (its last hop's column blocks + int32 flags); the peers map it once and
 * every call (1) computes a row chunk into that buffer, (2) raises the chunk's
 * flag to the call's sequence number (sgc_signal_flag_i32), (3) waits for every
 * peer's flag (sgc_wait_flags_i32) and (4) pulls all P blocks of the chunk
 * straight into X_K's columns (sgc_pull_blocks_f32).
 *
 * sgc_ipc_get_handle: the SGC_IPC_HANDLE_BYTES handle of the allocation that
 * holds `ptr` (hipIpcGetMemHandle) with ptr's offset in it.  sgc_ipc_open (in
 * another process): maps it; *base_host is what sgc_ipc_close takes, *ptr_host
 * the peer's pointer in this process. */
#define SGC_IPC_HANDLE_BYTES 128
int sgc_ipc_get_handle(const void *ptr, void *handle_host);
int sgc_ipc_open(const void *handle_host, void **base_host, void **ptr_host);
int sgc_ipc_close(void *base);
/* *flag = value once everything enqueued on `stream` before it is visible at
 * system scope (one-lane release store). */
int sgc_signal_flag_i32(int32_t *flag, int32_t value, void *stream);
/* The stream waits until flag_ptrs_host[i][0] >= value for every i < n (n <=
 * 64; one polling wave, acquire loads at system scope); after timeout_us it
 * stops waiting and sets *err = 1 (a host-visible word the caller checks after
 * synchronising: a lost peer never hangs the device). */
int sgc_wait_flags_i32(int32_t n, const int64_t *flag_ptrs_host, int32_t value, int32_t *err,
                       int64_t timeout_us, void *stream);
/* Batched 2-D block copy with one source pointer per segment (a peer's mapped
 * buffer or this rank's own): segs_host[6s .. 6s+5] = (src pointer, src row
 * stride in floats, dst_row, dst_col, rows, cols), nseg <= 16:
 *     dst[dst_row + i, dst_col + j] = src[i * lds + j];
 * sources read with system-coherent loads; a segment's source span must stay
 * below 2 GiB (split its rows). */
int sgc_pull_blocks_f32(int32_t nseg, const int64_t *segs_host, float *dst, int64_t ldd,
                        void *stream);

/* Recorded launch lists: the K-hop loop's launches (sgc_spmm_csr_f32_ex /
 * sgc_pad_rows_f32 with their arguments) recorded once and replayed by ONE
 * call per propagation -- at Pubmed shape the per-launch host cost (~4 us)
 * is a tenth of a hop.  A pointer argument of a recorded launch is either
 * fixed (SGC_SLOT_FIXED: the recorded pointer, e.g. an intermediate buffer the
 * caller keeps alive) or the run's X_0 / X_K (SGC_SLOT_X0 / SGC_SLOT_OUT: the
 * pointers given to sgc_launch_list_run), so one list serves every feature
 * tensor of the recorded shape, strides and alignment; each replayed launch
 * makes its kernel choice from the actual pointers, as a direct call does.
 * A list belongs to the device current at creation (the run switches to it
 * and back).  Runs, adds and destroys are serialised by one library lock
 * (a run is a few launches); one list must still not run concurrently on
 * two streams when it holds fixed intermediates.  No reference counterpart: the reference's
 * loop (utils.py:94-96) is one torch.spmm call per hop. */
enum { SGC_SLOT_FIXED = 0, SGC_SLOT_X0 = 1, SGC_SLOT_OUT = 2 };
int sgc_launch_list_create(int64_t *handle_host);
int sgc_launch_list_add_spmm(int64_t handle, const int32_t *row_ptr, const int32_t *col_idx,
                             const float *val, int64_t row_begin, int64_t row_end,
                             const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                             const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                             int32_t heavy_threshold, uint32_t flags, int32_t x_slot,
                             int32_t y_slot);
/* (records an sgc_spmm_csr_f32_ex2 launch: n_nonempty as there) */
int sgc_launch_list_add_spmm_ex2(int64_t handle, const int32_t *row_ptr,
                                 const int32_t *col_idx, const float *val, int64_t row_begin,
                                 int64_t row_end, const float *X, int64_t ldx, float *Y,
                                 int64_t ldy, int64_t F, const int32_t *plan, int64_t n_heavy,
                                 int64_t n_hub, int32_t heavy_threshold, uint32_t flags,
                                 int64_t n_nonempty, int32_t x_slot, int32_t y_slot);
/* (records an sgc_spmm_csr_f32_ex3 launch: n_not_wide / wide_max_nnz as there;
 * the "short_wide" knob is read when the list runs) */
int sgc_launch_list_add_spmm_ex3(int64_t handle, const int32_t *row_ptr,
                                 const int32_t *col_idx, const float *val, int64_t row_begin,
                                 int64_t row_end, const float *X, int64_t ldx, float *Y,
                                 int64_t ldy, int64_t F, const int32_t *plan, int64_t n_heavy,
                                 int64_t n_hub, int32_t heavy_threshold, uint32_t flags,
                                 int64_t n_nonempty, int64_t n_not_wide, int32_t wide_max_nnz,
                                 int32_t x_slot, int32_t y_slot);
int sgc_launch_list_add_pad_rows(int64_t handle, const float *src, int64_t lds, float *dst,
                                 int64_t ldd, int64_t n_rows, int64_t F, int32_t src_slot,
                                 int32_t dst_slot);
int sgc_launch_list_run(int64_t handle, const float *X0, float *out, void *stream);
int sgc_launch_list_destroy(int64_t handle);

/* The row stride (floats) the engine uses for its own feature buffers. */
int64_t sgc_aligned_ld(int64_t F);

/* One hop with the features stored in 16 bits: 16 bits in memory, fp32
 * everywhere else.  x_dtype = SGC_DTYPE_BF16 or SGC_DTYPE_F16 (torch.bfloat16
 * / torch.float16 bit patterns); y_dtype = x_dtype, or SGC_DTYPE_F32; S (val)
 * stays fp32.  ldx / ldy count elements of X's / Y's own type.  Every output
 * element is
 *     Y[i,f] = round_T(chain),  chain: acc = +0.0f; for k in row i, CSR order:
 *                                          acc = fmaf(val[k], (float)X[col[k],f], acc)
 * -- the single sequential fp32 FMA chain of sgc_spmm_csr_f32 (never split
 * across lanes or waves) on the exactly widened elements, rounded to nearest
 * even once per output element: for finite values the bits of torch's CPU
 * tensor.to(T), subnormal results and fp16 overflow to +-inf included; NaN
 * stays NaN (any payload).  With y_dtype = SGC_DTYPE_F32 the unrounded chain
 * is stored.  So a hop is bit-identical to
 *     sgc_spmm_csr_f32(S, (float)X) converted to T,
 * and a K-hop loop through 16-bit buffers to K such hops; the plan (plan,
 * n_heavy, n_hub, heavy_threshold, as sgc_spmm_csr_f32) is a schedule only.
 * Special values, as for sgc_spmm_csr_f32: NaN exactly where that definition
 * gives NaN (payload and sign unspecified), every other 16-bit pattern equal
 * -- signed zeros and the 16-bit format's subnormals included -- on every
 * schedule.
 * flags: the bits of sgc_spmm_csr_f32_ex.  For a 16-bit operand the padded
 * flags mean columns [F, round8(F)) (readable in X / writable in Y);
 * the 4 GiB flag means n_cols * ldx * 2 < 2^32; the accumulate flag
 * is accepted only with y_dtype = SGC_DTYPE_F32 (a chain carried through a
 * 16-bit store would not be exact) -- any other combination, or an unknown
 * dtype, returns SGC_EINVAL with an sgc_last_error text.
 * 16-byte lanes (8 elements) need 16-B aligned X rows (the engine's buffers:
 * rows of sgc_aligned_ld_x16(F) elements); any other even-byte layout -- an
 * odd ldx, a base that is only 2-B aligned -- runs on narrower loads with the
 * same bits.  Columns >= F are never stored, and never read unless the caller
 * set the padded flags. */
enum { SGC_DTYPE_F32 = 0, SGC_DTYPE_BF16 = 1, SGC_DTYPE_F16 = 2 };
int sgc_spmm_csr_x16(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                     int64_t row_begin, int64_t row_end,
                     const void *X, int32_t x_dtype, int64_t ldx,
                     void *Y, int32_t y_dtype, int64_t ldy, int64_t F,
                     const int32_t *plan, int64_t n_heavy, int64_t n_hub,
                     int32_t heavy_threshold, uint32_t flags, void *stream);

/* The row stride (16-bit elements) of the engine's own 16-bit feature
 * buffers: F rounded up to 64 elements (128-B rows). */
int64_t sgc_aligned_ld_x16(int64_t F);

/* ---------------------------------------------------------------------------
 * Classifier forward Y[M,C] = X[M,K] . W[C,K]^T + b[C]  (models.py:17-18,
 * nn.Linear) at fp32 precision on MFMA: where W's three bf16 images fit LDS
 * (e.g. K = 602, C <= 42) and M >= 4096, every operand is split exactly into
 * three bf16 pieces and the six products that reach fp32 precision run on
 * v_mfma_f32_16x16x32_bf16; otherwise fp32 MFMA (v_mfma_f32_16x16x4_f32).
 * b may be NULL.  X row stride ldx, Y row stride ldy.  Tolerance-equal to
 * torch (summation order differs), not bit-equal.
 * ------------------------------------------------------------------------- */
int sgc_linear_f32(const float *X, int64_t ldx, const float *W, const float *b,
                   float *Y, int64_t ldy, int64_t M, int64_t K, int64_t C, void *stream);

/* Name of the kernel sgc_linear_f32 launches for these arguments (under the
 * current "linear_kernel" tuning), for benchmark labels; "none" for an empty
 * or invalid shape.  Static storage. */
const char *sgc_linear_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C, const float *X);
/* The weight-backward kernel sgc_linear_backward_f32 runs for this shape /
 * alignment under the current "backward_kernel" tuning (static string; bench
 * labels); "none" for an empty or invalid shape. */
const char *sgc_linear_backward_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                            const float *X);

/* Backward of sgc_linear_f32 for the weights (what autograd runs for
 * nn.Linear after F.cross_entropy(model(x), y).backward() in the closures of
 * citation.py:47-49 and reddit.py:55-58):  dW[C,K] = dY^T X,  db[C] = sum_m dY
 * (db may be NULL), from one read of X on fp32 MFMA; dY [M,C] with row stride
 * ldd.  C <= 64.  Fixed-order reductions: bitwise reproducible run to run,
 * within fp32 tolerance of torch.  workspace: sgc_linear_backward_workspace
 * (M, K, C) bytes.  (dX = dY W, needed only when x requires a gradient, is
 * not computed here.) */
int64_t sgc_linear_backward_workspace(int64_t M, int64_t K, int64_t C);
int sgc_linear_backward_f32(const float *X, int64_t ldx, const float *dY, int64_t ldd,
                            int64_t M, int64_t K, int64_t C, float *dW, float *db,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* The classifier on 16-bit features: X is torch.bfloat16 / torch.float16
 * memory (x_dtype = SGC_DTYPE_BF16 / SGC_DTYPE_F16; anything else returns
 * SGC_EINVAL with an sgc_last_error text before any pointer is touched); W, b,
 * dY, Y, dW and db stay fp32.  Results are defined on the exactly widened
 * elements -- Y = float(X) W^T + b, dW = dY^T float(X), db = sum dY -- and
 * nothing is rounded to 16 bits: a bf16 x is one bf16 piece (3 MFMAs per class
 * tile, nothing dropped), an fp16 x exactly two (5 MFMAs), W and dY three as
 * in the fp32 kernels.  A non-finite x inside the K range gives non-finite
 * results in its row of Y / its column of dW, not necessarily torch's +-inf;
 * padding past K may hold anything.
 * Covered: even element pitch ldx, X 4-B aligned, M * ldx * 2 < 2^31, and for
 * the forward every class block (64 classes at a time) with its W image
 * within LDS (K = 602: C <= 42), at any M >= 1; for the backward C <= 48.
 * Anything else returns SGC_EINVAL and the name functions return "none":
 * there is no fp32 kernel behind these entry points.  workspace:
 * sgc_linear_backward_x16_workspace(M, K, C) bytes.  The unit is not part of
 * sgc_warmup. */
int sgc_linear_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                   float *Y, int64_t ldy, int64_t M, int64_t K, int64_t C, void *stream);
const char *sgc_linear_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                       const void *X, int32_t x_dtype);
int64_t sgc_linear_backward_x16_workspace(int64_t M, int64_t K, int64_t C);
int sgc_linear_backward_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *dY, int64_t ldd,
                            int64_t M, int64_t K, int64_t C, float *dW, float *db,
                            void *ws, int64_t ws_bytes, void *stream);
const char *sgc_linear_backward_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                                const void *X, int32_t x_dtype);

/* Softmax cross-entropy over a logits matrix: the loss the reference's
 * closures take of the classifier's output, F.cross_entropy(model(x), y)
 * with mean reduction (citation.py:46-49, reddit.py:55-58), and its
 * gradient.  logits [M, C] (row stride ldl, C <= 64), labels int64 [M]; rows
 * whose label equals ignore_index are left out of the mean (torch's
 * default is -100).  Forward: *loss = mean over the counted rows of
 * lse_m - logits[m, y_m], lse[m] = log sum_c exp(logits[m, c]) (an output;
 * the backward takes the pointer but recomputes the row's max and sum),
 * *inv_count = 1 / (counted rows); NaN loss for a label outside
 * [0, C).  Backward: dlogits = (softmax - onehot) * (*grad_loss) *
 * (*inv_count) (grad_loss may be NULL: 1), zero rows for ignored labels.
 * Device scalars throughout (no host synchronisation).  Deterministic;
 * tolerance-equal to torch (rtol 1e-5) whatever the logits' magnitude: the
 * loss term is (max - logits[m, y_m]) + log(sum) and the softmax
 * exp(logits - max) / sum, neither formed from the rounded lse.  workspace:
 * sgc_cross_entropy_workspace(M, C) bytes. */
int64_t sgc_cross_entropy_workspace(int64_t M, int64_t C);
int sgc_cross_entropy_f32(const float *logits, int64_t ldl, const int64_t *labels, int64_t M,
                          int64_t C, int64_t ignore_index, float *loss, float *inv_count,
                          float *lse, void *workspace, int64_t workspace_bytes, void *stream);
int sgc_cross_entropy_backward_f32(const float *logits, int64_t ldl, const int64_t *labels,
                                   const float *lse, const float *inv_count,
                                   const float *grad_loss, int64_t M, int64_t C,
                                   int64_t ignore_index, float *dlogits, int64_t ldd, void *stream);

/* ---------------------------------------------------------------------------
 * Fused classifier training step: for the SGC closure
 * (citation.py:46-49, reddit.py:55-58: F.cross_entropy(model(x), y) then
 * backward) computes, in three launches reading X twice,
 *     loss = mean_m [ logsumexp(z_m) - z_m[y_m] ],  z = X W^T + b
 *     dW   = (softmax(z) - onehot(y))^T X / M,     db = sum_m (...) / M
 * loss is one float; dW [C,K], db [C] (db may be NULL); logits [M,C] with row
 * stride ldl are written when non-NULL.  C <= 64.  Labels must lie in
 * [0, C) (not checked on the device; the Python layer checks them).  Reductions run in a fixed order:
 * results are bitwise reproducible run to run; within fp32 tolerance of torch.
 * workspace: sgc_linear_xent_workspace(M, K, C) bytes.
 * ------------------------------------------------------------------------- */
int64_t sgc_linear_xent_workspace(int64_t M, int64_t K, int64_t C);
int sgc_linear_xent_f32(const float *X, int64_t ldx, const float *W, const float *b,
                        const int64_t *labels, int64_t M, int64_t K, int64_t C, float *loss,
                        float *dW, float *db, float *logits, int64_t ldl, void *workspace,
                        int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Device-resident L-BFGS: replaces optim.LBFGS(lr=1).step(closure) of
 * reddit.py:51-64, the form with line_search_fn=None only.  torch's loop
 * synchronises with the host on every dot product and every termination
 * test; here the loop is cut at the closure boundary: after each closure one
 * launch (sgc_lbfgs_iterate_f32, one 1024-thread workgroup) runs the
 * termination tests of the iteration just taken and then the memory update,
 * the two-loop recursion, the step size and the in-place parameter update of
 * the next one.  A device stop word turns every later launch of the step
 * into a no-op, so the host reads the status once per step.
 *
 * Arithmetic: vectors fp32; every dot product, |g|_1, max|g| and max|t d| is
 * accumulated in fp64 in a fixed order from exact products of the fp32
 * elements and rounded to fp32 once; elementwise updates are single fmafs.
 * Bitwise reproducible run to run; tolerance-equal to torch, not bit-equal
 * (another summation order).  Every comparison takes torch's branch on NaN
 * (all false: a NaN loss or gradient stops nothing and pushes no pair).
 *
 *   sgc_lbfgs_workspace(n, history_size): bytes of the caller-owned device
 *     state (256-B aligned), 0 with an error text for n outside 1..65536 or
 *     history_size outside 1..1024.  Layout: a 256-B scalar block, then
 *     ro[history_size] (padded to 256 B), d[ld], prev_g[ld], S[history_size][ld],
 *     Y[history_size][ld] with ld = n rounded up to 32 floats (al of the
 *     two-loop recursion lives in LDS during a launch).  The scalar block
 *     starts with six int64 -- n_iter and func_evals (global, as torch's
 *     state), iters and evals (this step), stop (SGC_LBFGS_STOP_*), hist_len
 *     -- which sgc_lbfgs_read_status copies back; after them the ring head,
 *     n, history_size, ld (int64), loss and prev_loss (double), H_diag and t
 *     (float).
 *   sgc_lbfgs_init: zero the state and record its shape.  Asynchronous.
 *   sgc_lbfgs_begin_step: reset iters, evals and stop.  Asynchronous.
 *   sgc_lbfgs_iterate_f32: the launch above, after a closure.  n_tensors
 *     (1..16) contiguous fp32 parameter tensors of numels_host[i] elements
 *     (summing to the state's n) at param_ptrs_host[i], their gradients at
 *     grad_ptrs_host[i] (a NULL entry is a zero gradient, as torch
 *     substitutes for p.grad is None); the three host tables travel as kernel
 *     arguments.  loss: the closure's value, one device float.  Asynchronous,
 *     never synchronises.
 *   sgc_lbfgs_read_status: out_host[0..6) = n_iter, func_evals, iters, evals,
 *     stop reason, hist_len.  Synchronous.
 * Argument errors return SGC_EINVAL / SGC_ERANGE (n > 65536, history_size >
 * 1024) before any device call.
 * ------------------------------------------------------------------------- */
enum {
    SGC_LBFGS_STOP_NONE = 0,         /* the step is still running               */
    SGC_LBFGS_STOP_OPT_AT_ENTRY = 1, /* max|g| <= tolerance_grad, first closure */
    SGC_LBFGS_STOP_MAX_ITER = 2,     /* max_iter iterations taken               */
    SGC_LBFGS_STOP_MAX_EVAL = 3,     /* max_eval closures consumed              */
    SGC_LBFGS_STOP_OPT = 4,          /* max|g| <= tolerance_grad                */
    SGC_LBFGS_STOP_GTD = 5,          /* g.d > -tolerance_change, no update      */
    SGC_LBFGS_STOP_STEP_SMALL = 6,   /* max|t d| <= tolerance_change            */
    SGC_LBFGS_STOP_LOSS_CHANGE = 7   /* |loss - prev_loss| < tolerance_change   */
};
int64_t sgc_lbfgs_workspace(int64_t n, int32_t history_size);
int sgc_lbfgs_init(void *state, int64_t state_bytes, int64_t n, int32_t history_size,
                   void *stream);
int sgc_lbfgs_begin_step(void *state, void *stream);
int sgc_lbfgs_iterate_f32(void *state, int32_t n_tensors, float *const *param_ptrs_host,
                          const float *const *grad_ptrs_host, const int64_t *numels_host,
                          const float *loss, double lr, int32_t max_iter, int32_t max_eval,
                          double tolerance_grad, double tolerance_change, void *stream);
int sgc_lbfgs_read_status(const void *state, int64_t *out_host, void *stream);

/* ---------------------------------------------------------------------------
 * Fused L-BFGS training: `steps` times optim.LBFGS(lr).step(closure) of
 * reddit.py:51-64 for the SGC classifier z = X W^T + b, the closure
 * F.cross_entropy(z, labels) plus backward on the device side too.
 *
 *   sgc_train_lbfgs_f32: one host call enqueues everything on `stream`: no
 *     host synchronisation, no allocation, no atomics, every sum in a fixed
 *     order.  Per step: the reset of sgc_lbfgs_begin_step, then max_iter times
 *     [the closure: launches A and B of sgc_linear_xent_f32 and its two
 *     reductions, writing loss, dW and db into a flat gradient (W then b) in
 *     the workspace; then the launch of sgc_lbfgs_iterate_f32 on the tensors
 *     W, b and that gradient], then a one-thread launch that copies the six
 *     status words to status_trace.  Kernel selection is sgc_linear_xent_f32's
 *     (alignment of X, ldx, K and W; "backward_kernel" and "tile_buffers").
 *     The closure launches are stop-aware forms of sgc_linear_xent_f32's
 *     kernels: each tests the state's stop word with one wave-uniform load at
 *     entry and returns when it is set, so once a step has stopped its
 *     remaining iterations cost empty launches and move nothing; while the
 *     step runs they compute sgc_linear_xent_f32's bits.  The result -- W, b,
 *     the whole state, every status and loss -- is therefore bit-identical to
 *     the same steps driven closure by closure through sgc_linear_xent_f32 and
 *     sgc_lbfgs_iterate_f32.
 *     state: the sgc_lbfgs_workspace state, initialised by sgc_lbfgs_init with
 *     n = C*K + C (n = C*K when b is NULL); the flat vector is W then b.  The
 *     same state serves sgc_lbfgs_iterate_f32: fused and stepwise steps may
 *     alternate.  W [C, K] and b [C] are updated in place.
 *     loss_trace: `steps` device floats or NULL; loss_trace[s] is the loss of
 *     step s's first closure (what step() returns).  status_trace: 6 * steps
 *     device int64 or NULL; status_trace[6 s .. 6 s + 5] are the status words
 *     of sgc_lbfgs_read_status as they stand at the end of step s.  The
 *     caller copies the table back when it likes: the only read-back.
 *     Limits: those of the parts -- C <= 64, n <= 65536, ldx >= K, X 4-B
 *     aligned, the 31-bit offset limits of sgc_linear_xent_f32.  Labels must
 *     lie in [0, C) (not checked on the device; the Python layer checks them).
 *     steps == 0 returns SGC_OK and touches nothing.
 *   sgc_train_lbfgs_workspace(M, K, C): bytes of `workspace` -- the flat
 *     gradient, one loss float and sgc_linear_xent_workspace(M, K, C); 0 for an
 *     empty shape, C > 64 or C*K > 65536.
 * Argument errors return SGC_EINVAL / SGC_ERANGE / SGC_ENOMEM (workspace)
 * with an sgc_last_error text before any device call.
 * ------------------------------------------------------------------------- */
int64_t sgc_train_lbfgs_workspace(int64_t M, int64_t K, int64_t C);
int sgc_train_lbfgs_f32(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                        int64_t M, int64_t K, int64_t C, void *state, int32_t steps,
                        double lr, int32_t max_iter, int32_t max_eval,
                        double tolerance_grad, double tolerance_change,
                        float *loss_trace, int64_t *status_trace,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Wide L-BFGS: sgc_lbfgs_iterate_f32's contract for 1 <= n < 2^31 - 1
 * parameters (memory permitting), history_size 1..1024, spread over the
 * machine.  The two-loop recursion runs in coefficient space: the state keeps,
 * in fp64, every dot product between the basis vectors {s_i, y_i, g} (the Gram
 * block), and d is formed as one linear combination of the basis.  One
 * iteration is six launches whatever n and hist_len are; no host
 * synchronisation, no allocation, no atomics.  Status words, stop reasons, the
 * stop word's meaning, the NaN branches and the arithmetic contract (fp32
 * vectors, fp64 accumulation of exact products in a fixed order that depends
 * on n only, single-fmaf updates) are the narrow call's.  Results are bitwise
 * reproducible and tolerance-equal to torch and to the narrow call (the
 * recursion's intermediate q and r are never rounded to fp32 here).
 *
 *   sgc_lbfgs_wide_workspace(n, history_size): bytes of the state (0 and an
 *     sgc_last_error text when the shape is refused).  Layout, m =
 *     history_size, ld = n rounded up to 32 floats; the f32 rows are 128-B
 *     aligned (ld * 4 is a multiple of 128), every other block 256-B aligned
 *     and padded to a multiple of 256 B:
 *       header 256 B   the narrow header (the six status words, head, n,
 *                      history_size, ld, loss, prev_loss, H_diag, t), then the
 *                      hand-over words of the six launches
 *       ro[m] f32      1 / ys per ring slot
 *       d[ld], prev_g[ld], S[m][ld], Y[m][ld]   f32 rows, pad columns zero
 *       s_new[ld], y_new[ld]   the staged pair t d and g - prev_g: it enters
 *                      the ring only once accepted (ys > 1e-10), so a rejected
 *                      pair never touches the slot it would evict
 *       coef[2m+1] f64 the direction's coefficients, logical order (s, y, g)
 *       red[16+6m] f64 the summed dots of the last scan
 *       G[2m+1][2m+1] f64   the Gram block: index k < m is S slot k, m + k is
 *                      Y slot k, 2m is g (after an iteration: prev_g)
 *       partials[ceil(ld / tile)][16+6m] f64   per-workgroup partial dots;
 *                      tile = 1024 floats up to ld = 262,144, 2048 up to
 *                      1,048,576, 4096 above
 *   sgc_lbfgs_wide_init / _begin_step / _iterate_f32 / _read_status: arguments
 *     and errors as the narrow four, without the 65,536 limit.  The library
 *     remembers (address -> n, history_size) from init until init is called
 *     on that address again: a freed and reused address must be initialised
 *     anew before any other call, as for the narrow state.
 *   sgc_lbfgs_wide_sync_gram: recomputes every Gram entry from the rows as they
 *     lie in the state (prev_g as g), with the dot routine and order of the
 *     incremental path.  For a state whose rows the caller wrote (a state
 *     loaded from elsewhere); a state the iterations built never needs it.
 *   sgc_lbfgs_wide_l2_f32: the reference's L2 term (TextSGC train.py) on one
 *     tensor behind the state's stop word: grad += l2 W (one fmaf each) and
 *     *loss += (float)(0.5 l2 sum W^2), the sum in fp64 partials of 4096
 *     elements in order.  l2 == 0 enqueues nothing.  numel <= the state's n;
 *     uses the state's partials block, so it goes between the closure and
 *     sgc_lbfgs_wide_iterate_f32.
 *   sgc_train_lbfgs_wide_f32: sgc_train_lbfgs_f32's loop on the wide iteration:
 *     per step the reset, max_iter times [the closure of sgc_linear_xent_f32
 *     behind the stop word (C <= 64, its 31-bit offset limits), the L2 term on
 *     W (never on b) when l2 != 0, the iteration on [W] (b NULL) or [W, b]],
 *     the status snapshot.  loss_trace / status_trace as the narrow call.
 *     Bit-identical to the same steps driven call by call.
 * Argument errors return SGC_EINVAL / SGC_ERANGE / SGC_ENOMEM with an
 * sgc_last_error text before any device call.
 * ------------------------------------------------------------------------- */
int64_t sgc_lbfgs_wide_workspace(int64_t n, int32_t history_size);
int sgc_lbfgs_wide_init(void *state, int64_t state_bytes, int64_t n, int32_t history_size,
                        void *stream);
int sgc_lbfgs_wide_begin_step(void *state, void *stream);
int sgc_lbfgs_wide_iterate_f32(void *state, int32_t n_tensors, float *const *param_ptrs_host,
                               const float *const *grad_ptrs_host, const int64_t *numels_host,
                               const float *loss, double lr, int32_t max_iter, int32_t max_eval,
                               double tolerance_grad, double tolerance_change, void *stream);
int sgc_lbfgs_wide_read_status(const void *state, int64_t *out_host, void *stream);
int sgc_lbfgs_wide_sync_gram(void *state, void *stream);
int sgc_lbfgs_wide_l2_f32(void *state, const float *W, float *grad, int64_t numel, double l2,
                          float *loss, void *stream);
int64_t sgc_train_lbfgs_wide_workspace(int64_t M, int64_t K, int64_t C);
int sgc_train_lbfgs_wide_f32(const float *X, int64_t ldx, float *W, float *b,
                             const int64_t *labels, int64_t M, int64_t K, int64_t C, void *state,
                             int32_t steps, double lr, int32_t max_iter, int32_t max_eval,
                             double tolerance_grad, double tolerance_change, double l2,
                             float *loss_trace, int64_t *status_trace, void *workspace,
                             int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Device-resident Adam: optim.Adam of citation.py:41-50 (torch's default
 * single-tensor math: amsgrad=False, maximize=False, coupled L2 weight decay).
 *
 * Per element, in fp32 with one rounding per operation, in this order:
 *     g' = g + wd * p                       (skipped when wd == 0)
 *     m  = m + (g' - m) * (1 - b1)
 *     v  = b2 * v + ((1 - b2) * g') * g'
 *     denom = sqrt(v) / sqrt(1 - b2^step) + eps
 *     p  = p - (lr / (1 - b1^step)) * (m / denom)
 * wd, 1 - b1, b2, 1 - b2, eps, sqrt(1 - b2^step) and lr / (1 - b1^step) are
 * computed on the host in double and rounded to fp32 once; sqrt and the
 * divisions are correctly rounded, no product is contracted into a sum.
 * Bitwise reproducible run to run; tolerance-equal to torch, not bit-equal.
 *
 *   sgc_adam_step_f32: one launch updates n_tensors (1..16) contiguous fp32
 *     tensors of numels_host[i] elements, p, exp_avg and exp_avg_sq in place;
 *     the host tables travel as kernel arguments.  A NULL gradient entry
 *     skips that tensor entirely (torch skips a parameter whose .grad is
 *     None; its state does not move).  step: the count after this update
 *     (>= 1).  Asynchronous, never synchronises.
 *
 *   sgc_train_adam_f32: the loop of citation.py:44-50 -- zero_grad, model(x),
 *     F.cross_entropy, backward, Adam.step -- for the SGC classifier
 *     z = X W^T + b, `epochs` times, enqueued on `stream` by one host call: no
 *     host synchronisation, no allocation, no atomics, every sum in a fixed
 *     order.  Epoch e uses Adam step step0 + e + 1 (step0 >= 0).  W [C, K],
 *     b [C] and their moments are updated in place; b and its two moments
 *     may be NULL together.  loss_trace: `epochs` device floats or NULL;
 *     loss_trace[e] is the mean cross-entropy at the weights before epoch e's
 *     update.  C <= 64; labels must lie in [0, C) (not checked on the device;
 *     the Python layer checks them).  X needs a 4-B aligned base and
 *     ldx >= K only.  workspace: sgc_train_adam_workspace(M, K, C) bytes (0
 *     for an empty shape or C > 64).
 *     Two schedules (sgc_set_tuning "adam_kernel"): the general one, any M,
 *     is launches A and B of sgc_linear_xent_f32 and one launch that reduces
 *     the dW, db and loss partials in sgc_linear_xent_f32's orders and applies
 *     the update in the threads holding the finished gradient elements (three
 *     launches per epoch); the small one, M <= 313, runs two launches per
 *     epoch over 64-column blocks of K with plain fp32 fmaf sums (partial
 *     logits per block, then softmax, dW of the block over all rows and the
 *     update).  313 rows is what one workgroup's 160 KB of LDS hold of
 *     G = softmax - onehot ([M][65] floats at 64 classes) next to its X tile
 *     ([M][64]) and 2 KB of scratch: (163,840 - 2,048) / 516.  The two
 *     schedules sum in different orders: tolerance-equal, not bit-equal.
 * Argument errors return SGC_EINVAL / SGC_ERANGE / SGC_ENOMEM (workspace)
 * with an sgc_last_error text before any device call.
 * ------------------------------------------------------------------------- */
int sgc_adam_step_f32(int32_t n_tensors, float *const *param_ptrs_host,
                      const float *const *grad_ptrs_host, float *const *exp_avg_ptrs_host,
                      float *const *exp_avg_sq_ptrs_host, const int64_t *numels_host,
                      int64_t step, double lr, double beta1, double beta2, double eps,
                      double weight_decay, void *stream);
int64_t sgc_train_adam_workspace(int64_t M, int64_t K, int64_t C);
int sgc_train_adam_f32(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                       int64_t M, int64_t K, int64_t C,
                       float *exp_avg_W, float *exp_avg_sq_W, float *exp_avg_b, float *exp_avg_sq_b,
                       int64_t step0, int32_t epochs, double lr, double beta1, double beta2,
                       double eps, double weight_decay, float *loss_trace,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Weight-decay sweep: B independent SGC classifiers on the same X and labels,
 * each with its own initial weights and its own weight decay -- the trials of
 * the reference's tuning.py:26-33 as one batch.
 *
 *   sgc_train_adam_sweep_f32: sgc_train_adam_f32 for models i = 0 .. B-1 in
 *     one host call.  W [B, C, K], b [B, C] and the four moment tensors are
 *     contiguous stacks (b and its two moments NULL together);
 *     weight_decay_dev is B DEVICE floats, one decay per model, which the host
 *     never reads; loss_trace is [B, epochs] (loss_trace[i * epochs + e]) or
 *     NULL.  1 <= B <= 4096.  For every model the updated W[i], b[i], moments
 *     and loss trace are BIT-IDENTICAL to one sgc_train_adam_f32 call on that
 *     model alone with weight_decay = (double)weight_decay_dev[i] on the
 *     schedule this call ran (below); a model whose decay is 0.0f takes the
 *     "skipped when wd == 0" path.  Asynchronous, no allocation, no atomics,
 *     no host synchronisation, every sum in a fixed order.
 *     Schedule: where the small schedule can take the shape (M <= 313) and
 *     "adam_kernel" is not 1, its two launches per epoch run on a K-block x
 *     model grid, each model on its own partial-logit area and bias copy of the
 *     workspace ("adam_kernel" = 2 results).  The second launch has two forms
 *     with the same results ("adam_sweep_form"): fused, where every K-block's
 *     workgroup re-sums its model's partial logits and redoes the softmax, and
 *     split, where one workgroup per model does that once and stores
 *     G = (softmax - onehot) / M for a dW launch over K-block x model (three
 *     launches per epoch).  The batched schedule holds under "adam_kernel" = 0
 *     too, at every eligible shape: the auto rule of sgc_train_adam_f32 was
 *     measured for one model and no crossover has been measured for a batch.
 *     Everything else (M > 313, "adam_kernel" = 1) enqueues the general
 *     schedule model by model ("adam_kernel" = 1 results).  The read-only
 *     tuning word "adam_sweep_last" reports what the last call ran: 2 batched
 *     small, 1 general per model, 0 none yet.
 *   sgc_train_adam_sweep_workspace(B, M, K, C): bytes of `workspace`; 0 for an
 *     empty shape, C > 64 or B outside 1..4096.
 *   sgc_linear_eval_sweep_f32: sgc_linear_eval_f32 for B stacked models in one
 *     host call (its launch chain once per model on the one workspace,
 *     sgc_linear_eval_workspace(M, K, C) bytes): pred [B, M], confusion
 *     [B, C, C], counts [B, 2], loss [B], each NULL on its own as there;
 *     model i's outputs are bit-identical to sgc_linear_eval_f32 on model i.
 *     Coverage and errors are sgc_linear_eval_f32's; 1 <= B <= 4096.
 * Argument errors (B out of range, a null weight_decay_dev, ldx < K, a short
 * workspace, b and its moments not given together) return SGC_EINVAL /
 * SGC_ENOMEM with an sgc_last_error text before any device call.
 * ------------------------------------------------------------------------- */
int64_t sgc_train_adam_sweep_workspace(int64_t B, int64_t M, int64_t K, int64_t C);
int sgc_train_adam_sweep_f32(const float *X, int64_t ldx, float *W, float *b,
                             const int64_t *labels, int64_t B, int64_t M, int64_t K, int64_t C,
                             float *exp_avg_W, float *exp_avg_sq_W, float *exp_avg_b,
                             float *exp_avg_sq_b, int64_t step0, int32_t epochs, double lr,
                             double beta1, double beta2, double eps,
                             const float *weight_decay_dev, float *loss_trace,
                             void *workspace, int64_t workspace_bytes, void *stream);
int sgc_linear_eval_sweep_f32(const float *X, int64_t ldx, const float *W, const float *b,
                              const int64_t *labels, int64_t B, int64_t M, int64_t K, int64_t C,
                              int64_t *pred, int64_t *confusion, int64_t *counts, float *loss,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Fused training on 16-bit features: the step, the Adam epochs and the L-BFGS
 * steps above with X as torch.bfloat16 / torch.float16 rows (x_dtype
 * SGC_DTYPE_BF16 / SGC_DTYPE_F16, ldx in 16-bit ELEMENTS); W, b, the loss,
 * dW, db, the moments and the L-BFGS state stay fp32 and are the ones the
 * _f32 entries use.  Each call has its _f32 counterpart's argument list with
 * `const void *X, int32_t x_dtype` in place of `const float *X`; there is no
 * logits output (sgc_linear_x16 gives the logits).
 *
 *   sgc_linear_xent_x16: three launches, X read twice at 16 bits:
 *     A  logits float(x) . W^T + b by sgc_linear_x16's split-bf16 stream (one
 *        piece for bf16: 3 MFMAs per class tile; two for fp16: 5), each
 *        16-row tile followed at once by sgc_linear_xent_f32's row epilogue
 *        (same formulas): G = (softmax - onehot) / M to the workspace and ONE
 *        LOSS PARTIAL PER 16-ROW TILE, a double indexed by tile number (the
 *        waves take tiles dynamically, so a per-wave partial would differ run
 *        to run);
 *     B  sgc_linear_backward_x16's kernel on G: dW partials over column
 *        blocks x row ranges, db partials from the same G loads;
 *     C  one launch that reduces dW, db and the loss, each in a fixed order.
 *   sgc_train_adam_x16: sgc_train_adam_f32's general schedule -- per epoch A,
 *     B and C with the Adam update applied in place by the thread that holds
 *     the finished gradient element.  The small schedule is fp32-only: 16-bit
 *     X runs the general one under every "adam_kernel" setting, and
 *     "adam_kernel_last" reads 1 after such a call.
 *   sgc_train_lbfgs_x16: sgc_train_lbfgs_f32's loop with the closure A, B, C
 *     behind the state's stop word (every launch tests it with one
 *     wave-uniform load at entry and returns when it is set).  The state is
 *     sgc_lbfgs_init's; fused and stepwise steps may alternate on it.  The
 *     result -- W, b, the whole state, every status and every loss -- is
 *     bit-identical to the same steps driven closure by closure through
 *     sgc_linear_xent_x16 and sgc_lbfgs_iterate_f32.
 *
 * Coverage: sgc_linear_xent_x16_kernel_name is the one authority (host only,
 * dereferences nothing, "none" outside coverage).  It covers exactly the
 * arguments for which sgc_linear_x16_kernel_name and
 * sgc_linear_backward_x16_kernel_name both name a kernel: bf16 or fp16, even
 * ldx >= K, X 4-B aligned, M * ldx * 2 < 2^31, W's operand image within LDS
 * (launch A needs what sgc_linear_x16 needs: no further margin), C <= 48.
 * sgc_train_lbfgs_x16 further needs C * K + C <= 65,536 (the L-BFGS state).
 * Outside coverage -- an unknown dtype and an odd ldx included -- the calls
 * return SGC_EINVAL with an sgc_last_error text before any pointer is touched,
 * and there is no fp32 kernel behind these entry points.  The workspace
 * functions return 0 where no layout of (M, K, C) is covered.  epochs == 0 /
 * steps == 0 with valid arguments return SGC_OK and enqueue nothing.
 *
 * Contracts, as the fp32 entries': no host synchronisation, no allocation, no
 * atomics on global memory; every sum in a fixed order, results bitwise
 * reproducible run to run; results defined on the exactly widened elements
 * (tolerance-equal to torch on X.float()); a non-finite x follows the
 * deviation documented for sgc_linear_x16.  Labels must lie in [0, C).
 * ------------------------------------------------------------------------- */
int64_t sgc_linear_xent_x16_workspace(int64_t M, int64_t K, int64_t C);
int sgc_linear_xent_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                        const int64_t *labels, int64_t M, int64_t K, int64_t C, float *loss,
                        float *dW, float *db, void *ws, int64_t ws_bytes, void *stream);
const char *sgc_linear_xent_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                            const void *X, int32_t x_dtype);
int64_t sgc_train_adam_x16_workspace(int64_t M, int64_t K, int64_t C);
int sgc_train_adam_x16(const void *X, int32_t x_dtype, int64_t ldx, float *W, float *b,
                       const int64_t *labels, int64_t M, int64_t K, int64_t C,
                       float *exp_avg_W, float *exp_avg_sq_W, float *exp_avg_b, float *exp_avg_sq_b,
                       int64_t step0, int32_t epochs, double lr, double beta1, double beta2,
                       double eps, double weight_decay, float *loss_trace,
                       void *workspace, int64_t workspace_bytes, void *stream);
int64_t sgc_train_lbfgs_x16_workspace(int64_t M, int64_t K, int64_t C);
int sgc_train_lbfgs_x16(const void *X, int32_t x_dtype, int64_t ldx, float *W, float *b,
                        const int64_t *labels, int64_t M, int64_t K, int64_t C, void *state,
                        int32_t steps, double lr, int32_t max_iter, int32_t max_eval,
                        double tolerance_grad, double tolerance_change, float *loss_trace,
                        int64_t *status_trace, void *workspace, int64_t workspace_bytes,
                        void *stream);

/* ---------------------------------------------------------------------------
 * Device-resident evaluation: what the reference's test_regression takes from
 * model(x) -- accuracy(output, labels) (citation.py:64-66), f1(output, labels)
 * (reddit.py:69-71), and the mean cross-entropy TextSGC's eval_linear adds --
 * from one launch chain that reads X once (at 16 bits where X is 16-bit) and
 * never forms the [M, C] logits:
 *     pred[m]         = argmax_c z[m, c],  z = X W^T + b         int64 [M]
 *     confusion[y][p] = #{m : labels[m] = y, pred[m] = p}         int64 [C][C]
 *                       (row = label, column = prediction: sklearn's layout)
 *     counts          = {rows counted, rows with pred = label}    int64 [2]
 *     loss            = mean_m [ (max_c z - z[y_m]) + log sum_c exp(z - max) ]
 * Accuracy is counts[1] / counts[0] (the matrix's trace over its sum); micro
 * and macro F1 follow from the matrix (sgc_amd.metrics.f1_from_confusion).
 *
 * Argmax rule: torch's max(1)[1] -- the smallest class index whose logit no
 * other class exceeds; a NaN logit counts as greater than everything, so the
 * first NaN wins; -0 and +0 tie.
 *
 * Launches: A the forward (sgc_linear_xent_f32's launch A for fp32 X: fp32 MFMA
 * on the 128-row LDS tile, any 4-B-aligned X; sgc_linear_x16's persistent
 * split-bf16 stream for 16-bit X) with the row epilogue for the argmax and the
 * loss term, storing 8 bytes per row; B labels x predictions into
 * workgroup-local LDS integer counters, one partial table per workgroup; C the
 * tables summed in workgroup order and the loss partials (double; one per
 * wave for fp32, ONE PER 16-ROW TILE indexed by tile number for 16-bit X, whose
 * waves take tiles dynamically) in a fixed order.  B is skipped without
 * confusion and counts, B and C without labels.
 *
 * Arguments: b may be NULL.  labels NULL means predictions only: confusion,
 * counts and loss must then be NULL.  Each of pred, confusion, counts and loss
 * may be NULL on its own (all four NULL is SGC_EINVAL).  A label outside
 * [0, C) leaves its row out of the matrix and the counts and makes the loss
 * NaN; it never indexes the matrix.  Every pointer is a device pointer.
 *
 * Coverage: the two name functions are the authority (host only, they
 * dereference nothing, "none" outside coverage).
 *   _f32: 1 <= C <= 64, ldx >= K, X 4-B aligned, M * ldx * 4 < 2^31
 *         (sgc_linear_xent_f32's limits);
 *   _x16: what sgc_linear_x16_kernel_name covers (bf16 or fp16, even ldx >= K,
 *         X 4-B aligned, M * ldx * 2 < 2^31, W's image within LDS) and
 *         C <= 64: one class block (K = 602 gives C <= 42).
 * Outside coverage the calls return SGC_EINVAL, and SGC_ENOMEM for a short
 * workspace, with an sgc_last_error text before any pointer is touched; there
 * is no other kernel behind these entries.  The workspace functions return 0
 * where no layout of (M, K, C) is covered.
 *
 * Contracts: asynchronous on `stream`, no host synchronisation, no
 * allocation, no atomics on global memory; the integer outputs are exact and
 * the loss is summed in a fixed order: every output is bitwise reproducible run
 * to run.  Logits within the classifier's fp32 tolerance of torch (rows whose
 * two largest logits lie closer than that may take either class); the loss
 * within rtol 1e-5.  A non-finite x follows the deviation documented for
 * sgc_linear_x16 / the split kernels: its row's prediction is then some class
 * in [0, C) and nothing else is disturbed.  The workspace holds the loss
 * partials, the counter tables and 8 M bytes of predictions that the counting
 * launch reads when the caller passes no `pred`; nothing of size M * C exists
 * anywhere in the call.  The two units are not part of sgc_warmup: a process's
 * first call pays their code-object load.
 * ------------------------------------------------------------------------- */
int64_t sgc_linear_eval_workspace(int64_t M, int64_t K, int64_t C);
int sgc_linear_eval_f32(const float *X, int64_t ldx, const float *W, const float *b,
                        const int64_t *labels, int64_t M, int64_t K, int64_t C,
                        int64_t *pred, int64_t *confusion, int64_t *counts, float *loss,
                        void *workspace, int64_t workspace_bytes, void *stream);
const char *sgc_linear_eval_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                        const float *X);
int64_t sgc_linear_eval_x16_workspace(int64_t M, int64_t K, int64_t C);
int sgc_linear_eval_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                        const int64_t *labels, int64_t M, int64_t K, int64_t C,
                        int64_t *pred, int64_t *confusion, int64_t *counts, float *loss,
                        void *workspace, int64_t workspace_bytes, void *stream);
const char *sgc_linear_eval_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                            const void *X, int32_t x_dtype);

/* ---------------------------------------------------------------------------
 * Host (CPU) twins, for CPU tensors: the reference runs utils.py:92-97 on the
 * CPU whenever CUDA is off (args.py:39 --no-cuda; load_citation(cuda=False)).
 * Every pointer here is a HOST pointer; the calls are synchronous and
 * thread-safe (no shared state).  Same numerical contract as the GPU entry
 * points: bit-identical to torch.spmm's CPU kernel.  n_threads <= 0 = all
 * hardware threads; threads own whole rows.
 *
 * sgc_coo_to_csr_cpu: as sgc_coo_to_csr (stable by row, no coalescing;
 *   status bits 1/2/4), SGC_ERANGE on an out-of-range index.
 * sgc_spmm_csr_f32_cpu: as sgc_spmm_csr_f32 (utils.py:95), no plan.
 * sgc_spmm_csr_f32_cpu_ex: with flags; SGC_SPMM_ACCUMULATE as on the GPU,
 *   the padding flags accepted (and unused), the hub-split flags rejected.
 * sgc_propagate_f32_cpu: as sgc_propagate_f32 (utils.py:92-97); workspace
 *   = sgc_propagate_cpu_workspace(n_rows, F, K) bytes of host memory.
 * ------------------------------------------------------------------------- */
int sgc_coo_to_csr_cpu(const int64_t *rows, const int64_t *cols, const float *vals,
                       int64_t nnz, int64_t n_rows, int64_t n_cols,
                       int32_t *row_ptr, int32_t *col_idx, float *val_out,
                       uint32_t *status_host);
int sgc_spmm_csr_f32_cpu(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                         int64_t row_begin, int64_t row_end,
                         const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                         int32_t n_threads);
int sgc_spmm_csr_f32_cpu_ex(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                            int64_t row_begin, int64_t row_end,
                            const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                            uint32_t flags, int32_t n_threads);
int64_t sgc_propagate_cpu_workspace(int64_t n_rows, int64_t F, int32_t K);
int sgc_propagate_f32_cpu(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                          int64_t n_rows, const float *X0, int64_t ldx, float *out,
                          int64_t ldo, int64_t F, int32_t K, void *workspace,
                          int64_t workspace_bytes, int32_t n_threads);

/* The whole launch plan in one call, on the device: plan[0 .. n) = every row
 * of [row_begin, row_end) sorted by degree, longest first, ties in ascending
 * row order (a stable radix sort) -- i.e. the heavy rows (degree > threshold)
 * heaviest first followed by the light rows in SGC_SPMM_LIGHT_ORDER order,
 * exactly what sgc_plan_build + sgc_plan_light_order write together.
 * counts_host[0] = rows above threshold (n_heavy), [1] = rows above
 * hub_threshold (n_hub), [2] = the longest row's nonzeros.  Synchronous (two
 * stream synchronisations: the counts, then the sort); workspace of
 * sgc_plan_sorted_workspace(n) bytes on the device.  Replaces nothing in the
 * reference (a schedule). */
int64_t sgc_plan_sorted_workspace(int64_t n_rows);
int sgc_plan_sorted(const int32_t *row_ptr, int64_t row_begin, int64_t row_end,
                    int32_t threshold, int32_t hub_threshold, int32_t *plan, void *workspace,
                    int64_t workspace_bytes, int64_t *counts_host, void *stream);
/* The same with a fourth count: counts_host[3] = rows of the range with at
 * least one nonzero.  The sorted plan's empty rows are its tail, so an
 * SGC_SPMM_ACCUMULATE launch given this count (sgc_spmm_csr_f32_ex2) stops
 * before them.  counts_host holds four values here. */
int sgc_plan_sorted_ex(const int32_t *row_ptr, int64_t row_begin, int64_t row_end,
                       int32_t threshold, int32_t hub_threshold, int32_t *plan, void *workspace,
                       int64_t workspace_bytes, int64_t *counts_host, void *stream);
/* The same with four more counts: counts_host[4..7] = rows of the range with
 * more than 4 / 8 / 16 / 32 nonzeros (heavy rows among them).  Longest first,
 * the non-empty rows of at most Ts nonzeros are the stretch just before the
 * empty tail: a launch with wide items (sgc_spmm_csr_f32_ex3) takes
 * n_not_wide = counts_host[4 + i] - n_heavy for Ts = 4 << i, so the
 * "short_wide" knob moves without a new plan.  counts_host holds eight
 * values here; the workspace is sgc_plan_sorted_workspace's. */
int sgc_plan_sorted_ex2(const int32_t *row_ptr, int64_t row_begin, int64_t row_end,
                        int32_t threshold, int32_t hub_threshold, int32_t *plan, void *workspace,
                        int64_t workspace_bytes, int64_t *counts_host, void *stream);

/* ---------------------------------------------------------------------------
 * Column groups of S (a schedule for the SpMM of utils.py:95; results
 * unchanged).  Splits every row's nonzeros at the column cuts
 * 0 = cuts[0] <= cuts[1] <= ... <= cuts[G] = n_cols into G CSRs over the same
 * rows.  REQUIRES rows whose columns do not decrease (sgc_coo_to_csr status
 * bit 2): group g's part of a row is then one contiguous run, the runs come
 * in group order, and a hop computed as G launches -- group 0 plain, groups
 * 1.. with SGC_SPMM_ACCUMULATE -- applies every row's FMAs in CSR order: the
 * same bits as one launch, while each launch gathers only its group's X rows
 * (a live X slice 1/G as large, more of it in the per-XCD L2s).
 *   row_ptrs: [G][n_rows+1] int32, group g's row_ptr at row_ptrs + g*(n_rows+1),
 *             absolute offsets into col_out/val_out (groups stored one after
 *             the other), so (row_ptrs + g*(n_rows+1), col_out, val_out) is an
 *             ordinary CSR for sgc_spmm_csr_f32_ex / sgc_plan_sorted;
 *   col_out / val_out: [nnz];  G <= 8;  asynchronous on `stream`;
 *   workspace: sgc_colsplit_workspace(n_rows, G) bytes on the device.
 * sgc_csr_colsplit_ex, whole_rows = T >= 0: a row of at most T nonzeros is not
 * cut -- its entire run goes to group 0, whatever its columns, and groups 1..
 * hold nothing of it.  A group costs per row (a wave slot, a read + write of
 * the row's partial sums, one more latency chain) and gains per gathered
 * nonzero; short rows are most rows and few nonzeros, and a whole row in
 * group 0 is that row's CSR chain in one launch, so the bits are the same.
 * Same layout and workspace; sgc_csr_colsplit is whole_rows = 0.
 * sgc_csr_colsplit_ex2, coarse_rows = H >= T and coarse_groups = Gc >= 1
 * dividing G: the rows above T are cut by length class.  A row of more than H
 * nonzeros is cut at all G cuts.  A row of T+1..H nonzeros is cut only at the
 * Gc coarse cuts -- coarse cut j is cuts[j * (G / Gc)] -- and the run of its
 * coarse range j is stored in group j * (G / Gc); every other group holds
 * nothing of it.  Long rows hold most nonzeros in few rows, so the fine cut
 * (a smaller live X slice per launch) costs them almost nothing per row; a
 * medium row keeps runs long enough to pay for its wave.  Each row's runs
 * still come in ascending group order, each contiguous: the same bits.  Same
 * layout and workspace; sgc_csr_colsplit_ex is Gc = G (H is then unused).
 * SGC_EINVAL (nothing launched) when Gc < 1, Gc does not divide G or H < T.
 * ------------------------------------------------------------------------- */
int64_t sgc_colsplit_workspace(int64_t n_rows, int32_t groups);
int sgc_csr_colsplit(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                     int64_t n_rows, int64_t n_cols, int32_t groups, const int32_t *cuts_host,
                     int32_t *row_ptrs, int32_t *col_out, float *val_out, void *workspace,
                     int64_t workspace_bytes, void *stream);
int sgc_csr_colsplit_ex(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                        int64_t n_rows, int64_t n_cols, int32_t groups,
                        const int32_t *cuts_host, int32_t whole_rows, int32_t *row_ptrs,
                        int32_t *col_out, float *val_out, void *workspace,
                        int64_t workspace_bytes, void *stream);
int sgc_csr_colsplit_ex2(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                         int64_t n_rows, int64_t n_cols, int32_t groups,
                         const int32_t *cuts_host, int32_t whole_rows, int32_t coarse_rows,
                         int32_t coarse_groups, int32_t *row_ptrs, int32_t *col_out,
                         float *val_out, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * One process, several GPUs (the multi-GPU form of the one
 * call reddit.py:43 makes, sgc_precompute -> utils.py:92-97).  The engine
 * splits the feature columns over the devices: device d pulls its column
 * block of X_0 from the home device (peer reads over xGMI), runs all K hops
 * over its own replica of S (no exchange between hops: column f of X_{k+1}
 * depends on column f of X_k only) and stores its block of X_K straight into
 * `out` on the home device.  Bit-identical to sgc_propagate_f32.
 *   sgc_mgpu_init(ndev, devices): devices[0] = home device (where the CSR,
 *     X_0 and out live); enables peer access between every pair, one stream
 *     per entry.  An index may repeat (virtual devices sharing one GPU).
 *     Re-initialising frees the previous engine and its attachments.
 *   sgc_mgpu_attach: replicate the CSR (home-device pointers, n_rows square)
 *     to every other device -- synchronous, once per adjacency -- and return
 *     a handle.  The caller keeps the home arrays alive until detach.
 *   sgc_mgpu_propagate: X_K = S^K X_0 (K >= 1) into out (row stride ldo),
 *     asynchronous on `stream` (home device): every device waits for the work
 *     already on `stream`, and `stream` waits for every device.
 *   sgc_mgpu_detach / sgc_mgpu_finalize: free one attachment / everything.
 * Replaces: the torch.spmm loop of utils.py:94-95 spread over the node. */
int sgc_mgpu_init(int ndev, const int *devices);
int sgc_mgpu_attach(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                    int64_t n_rows, int64_t nnz, void *stream, int64_t *handle);
int sgc_mgpu_propagate(int64_t handle, const float *X0, int64_t ldx, float *out, int64_t ldo,
                       int64_t F, int32_t K, void *stream);
int sgc_mgpu_detach(int64_t handle);
int sgc_mgpu_finalize(void);

/* ---------------------------------------------------------------------------
 * Process warm-up (replaces nothing in the reference; a one-time cost the
 * reference's first torch.spmm pays inside torch).  The HIP runtime loads a
 * translation unit's code object on the first launch of any of its kernels;
 * sgc_warmup launches one empty kernel per unit selected in `units` on
 * `stream` (the current device) and waits for them, so those loads happen
 * here rather than inside the first sgc_precompute the caller times
 * (reddit.py:43,72-74).  Units: SGC_WARM_PROPAGATE = SpMM, ingest, plan,
 * sort, column groups, the exchanges' block copy; SGC_WARM_CLASSIFIER = linear, fused loss, cross-entropy, L-BFGS, Adam;
 * SGC_WARM_LOADERS = normalisation, sub-graph.  Synchronous. */
enum { SGC_WARM_PROPAGATE = 1, SGC_WARM_CLASSIFIER = 2, SGC_WARM_LOADERS = 4 };
int sgc_warmup(uint32_t units, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGC_AMD_H */
