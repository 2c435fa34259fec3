// internal.h -- every declaration shared between the library's translation
// units, once: included by the file that defines each function and by its
// callers, so a drifted parameter, default or return type does not compile.
#pragma once

#include "common.h"

namespace sgc {

// One fp32 SpMM launch: sgc_spmm_csr_f32_ex3's arguments (include/sgc_amd.h).
// The narrower exported generations leave the neutral defaults.
struct SpmmCall {
    const int32_t *row_ptr, *col_idx;
    const float *val;
    int64_t row_begin, row_end;
    const float *X;
    int64_t ldx;
    float *Y;
    int64_t ldy, F;
    const int32_t *plan;
    int64_t n_heavy, n_hub;
    int32_t heavy_threshold;
    uint32_t flags;
    int64_t n_nonempty = -1;  // the plan's rows with nonzeros, -1 unknown
    int64_t n_not_wide = -1;  // its light rows above wide_max_nnz, -1 none
    int32_t wide_max_nnz = 0;
};
int launch_spmm(const SpmmCall &call, hipStream_t stream);
// host only: the schedule the call would take (sgc_spmm_kernel_name)
const char *spmm_kernel_name(const SpmmCall &call);
// the hub launch's side stream (spmm.hip): fork the light kernel's stream off
// `stream`, join it back (every fork is joined)
int fork_light_stream(hipStream_t stream, hipStream_t *light, void **side);
int join_light_stream(void *side, hipStream_t stream);

// Code-object warm-up, one per translation unit (SGC_WARM_UNIT, common.h)
hipError_t warm_spmm(hipStream_t);
hipError_t warm_side_streams();  // creates the SpMM's per-device side-stream pool
hipError_t warm_ingest(hipStream_t);
hipError_t warm_plan(hipStream_t);
hipError_t warm_sort(hipStream_t);
hipError_t warm_groups(hipStream_t);
hipError_t warm_exchange(hipStream_t);
hipError_t warm_linear(hipStream_t);
hipError_t warm_xent(hipStream_t);
hipError_t warm_xent_fwd_stop(hipStream_t);
hipError_t warm_loss(hipStream_t);
hipError_t warm_lbfgs(hipStream_t);
hipError_t warm_normalize(hipStream_t);
hipError_t warm_subgraph(hipStream_t);
hipError_t warm_adam(hipStream_t);

// Tuning knobs that live outside spmm.hip (sgc_set_tuning's table points at them).
// LDS image depth of the classifier tile (gemm_tile.h; linear.hip defines it,
// sgc_set_tuning("tile_buffers") sets it: 1 or 2).
extern int g_tile_buffers;
// Classifier forward kernel (linear.hip): 0 auto, 1 LDS tile, 2 streaming.
extern int g_linear_kernel;
// k per chunk of the streaming classifier kernel (32 or 64).
extern int g_linear_ck;
// Classifier weight backward: 0 auto, 1 fp32 MFMA slabs, 2 split-bf16 slabs (xent.hip).
extern int g_backward_kernel;
extern int g_x16_vec, g_x16_step;              // spmm16.hip
extern int g_adam_kernel, g_adam_kernel_last, g_adam_sweep_last;  // adam.hip
extern int g_adam_sweep_form, g_adam_sweep_form_last;

// sort.hip -- the library's own stable radix sort.
// Bytes of device workspace radix_sort_pairs needs for n pairs.
int64_t radix_sort_workspace(int64_t n);
// Stable LSD radix sort of n (key, value) pairs by key: ascending, or
// descending when `descending` (keys compared as key_max - key, so ties keep
// their input order either way).  Every key must be <= key_max; the number of
// 11-bit passes follows key_max.  keys_out / vals_out must not alias the
// inputs.  Asynchronous on `stream`; no host synchronisation.
int radix_sort_pairs(const uint32_t *keys_in, const int32_t *vals_in, uint32_t *keys_out,
                     int32_t *vals_out, int64_t n, uint32_t key_max, bool descending, void *ws,
                     int64_t ws_bytes, hipStream_t stream);

// plan.hip: the sorted plan with its kPlanSortedCounts counts (sgc_plan_sorted_ex2)
constexpr int kPlanSortedCounts = 8;
int plan_sorted(const int32_t *row_ptr, int64_t row_begin, int64_t row_end, int32_t threshold,
                int32_t hub_threshold, int32_t *plan, void *workspace, int64_t workspace_bytes,
                int64_t *counts_host, hipStream_t stream);
// groups.hip: the column split with the length ladder (sgc_csr_colsplit_ex2)
int colsplit(const int32_t *row_ptr, const int32_t *col_idx, const float *val, int64_t n_rows,
             int64_t n_cols, int32_t groups, const int32_t *cuts_host, int32_t whole_rows,
             int32_t coarse_rows, int32_t coarse_groups, int32_t *row_ptrs, int32_t *col_out,
             float *val_out, void *workspace, int64_t workspace_bytes, hipStream_t stream);
int csr_cols_ascending(const int32_t *row_ptr, const int32_t *col_idx, int64_t n_rows,
                       hipStream_t stream, bool *ascending);
int column_groups_rule(int64_t nnz, int64_t width);

// linear.hip / xent.hip / xent_fwd_stop.hip helpers of the other classifier units
// a workspace section's size: the next section starts 256-B aligned
inline int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }
hipError_t persistent_setup(const void *kernel, int *cus);
// xent.hip: the fixed-order reduction of the dW / db partials
hipError_t launch_reduce_dw_db(const float *slab, int n_parts, int C, int K, int C16, float *dW,
                               const float *db_slab, float *db, hipStream_t s);
// launch A behind the stop word: xent_fwd_kernel<V, NT, g_tile_buffers, StopWord>
// (xent_fwd.h, instantiated in xent_fwd_stop.hip)
hipError_t launch_xent_fwd_stop(int V, int NT, const int64_t *stop, const float *X, int64_t ldx,
                                const float *W, const float *b, const int64_t *labels, int M, int K,
                                int C, float *G, int ldg, double *loss_part, float *db_part,
                                float *logits, int64_t ldl, hipStream_t s);
int xent_closure_check(const char *what, int64_t M, int64_t K, int64_t C, int64_t ldx);
int xent_closure(const int64_t *stop, const float *X, int64_t ldx, const float *W, const float *b,
                 const int64_t *labels, int64_t M, int64_t K, int64_t C, float *loss, float *dW,
                 float *db, void *ws, hipStream_t s);
// xent.hip: one epoch of the general schedule (launches A and B of the fused
// classifier step, then the reduce + Adam kernel).  Arguments as
// sgc_train_adam_f32; ws as linear_xent_f32's.  wd_dev non-null: the weight
// decay is the device float *wd_dev (read by the last launch) and coef.wd is
// ignored -- sgc_train_adam_sweep_f32's per-model decays.
struct AdamCoef;  // adam_update.h
int xent_adam_epoch(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                    int64_t M, int64_t K, int64_t C, float *mW, float *vW, float *mb, float *vb,
                    const AdamCoef &coef, float *loss_out, void *ws, int64_t ws_bytes,
                    hipStream_t s, const float *wd_dev = nullptr);
int xent_adam_check(int64_t M, int64_t K, int64_t C, int64_t ldx);

int coo_to_csr_workspace(int64_t n_rows, int64_t nnz, size_t *bytes);
int coo_to_csr(const int64_t *rows, const int64_t *cols, const float *vals, int64_t nnz,
               int64_t n_rows, int64_t n_cols, int32_t *row_ptr, int32_t *col_idx,
               float *val_out, void *ws, size_t ws_bytes, uint32_t *status_host,
               hipStream_t stream);
int csr64_to_csr(const int64_t *crow, const int64_t *col, const float *vals, int64_t nnz,
                 int64_t n_rows, int64_t n_cols, int32_t *row_ptr, int32_t *col_idx,
                 float *val_out, uint32_t *status_host, hipStream_t stream);
int build_plan(const int32_t *row_ptr, int64_t row_begin, int64_t row_end, int32_t threshold,
               int32_t hub_threshold, int32_t *plan, int64_t capacity, int64_t *n_heavy_host,
               int64_t *n_hub_host, hipStream_t stream);
int light_order(const int32_t *row_ptr, int64_t row_begin, int64_t row_end, int32_t threshold,
                int32_t *light, int64_t *n_light_host, hipStream_t stream);
int launch_spmm_x16(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                    int64_t row_begin, int64_t row_end, const void *X, int32_t x_dtype,
                    int64_t ldx, void *Y, int32_t y_dtype, int64_t ldy, int64_t F,
                    const int32_t *heavy_rows, int64_t n_heavy, int64_t n_hub,
                    int32_t heavy_threshold, uint32_t flags, hipStream_t stream);
int launch_pad_rows(const float *src, int64_t lds, float *dst, int64_t ldd, int64_t n_rows,
                    int64_t F, hipStream_t stream);
int launch_copy_blocks(const float *src, int64_t lds, float *dst, int64_t ldd, int32_t nseg,
                       const int64_t *segs, hipStream_t stream);
int launch_pull_blocks(int32_t nseg, const int64_t *segs, float *dst, int64_t ldd,
                       hipStream_t stream);
int launch_wait_flags(int32_t n, const int64_t *flags, int32_t value, int32_t *err,
                      int64_t timeout_us, hipStream_t stream);
int launch_signal_flag(int32_t *flag, int32_t value, hipStream_t stream);
int ipc_get_handle(const void *ptr, void *handle);
int ipc_open(const void *handle, void **base, void **ptr);
int ipc_close(void *base);
size_t augnorm_scan_temp_bytes(int64_t n);
int augnorm_count(const int32_t *row_ptr, const int32_t *col, const double *val, int64_t n,
                  int64_t nnz, int32_t *out_row_ptr, double *rowsum, void *ws, size_t ws_bytes,
                  int64_t *out_nnz_host, uint32_t *status_host, hipStream_t s);
int augnorm_fill(const int32_t *row_ptr, const int32_t *col, const double *val, int64_t n,
                 const double *d, int32_t *out_row_ptr, int32_t *out_col, float *out_val,
                 void *ws, size_t ws_bytes, int64_t *out_nnz_host, hipStream_t s);
int csr_to_coo64(const int32_t *row_ptr, const int32_t *col, int64_t n, int64_t *rows64,
                 int64_t *cols64, hipStream_t s);
int64_t xent_workspace_bytes(int64_t M, int64_t K, int64_t C);
int linear_xent_f32(const float *X, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, float *loss,
                    float *dW, float *db, float *logits, int64_t ldl, void *ws, int64_t ws_bytes,
                    hipStream_t s);
int64_t cross_entropy_workspace(int64_t M, int64_t C);
int cross_entropy_fwd_f32(const float *Y, int64_t ldy, const int64_t *labels, int64_t M, int64_t C,
                          int64_t ignore_index, float *loss, float *inv_count, float *lse, void *ws,
                          int64_t ws_bytes, hipStream_t s);
int cross_entropy_bwd_f32(const float *Y, int64_t ldy, const int64_t *labels, const float *lse,
                          const float *inv_count, const float *grad, int64_t M, int64_t C,
                          int64_t ignore_index, float *dY, int64_t lddy, hipStream_t s);
int64_t linear_backward_workspace_bytes(int64_t M, int64_t K, int64_t C);
int linear_backward_f32(const float *X, int64_t ldx, const float *dY, int64_t ldd, int64_t M,
                        int64_t K, int64_t C, float *dW, float *db, void *ws, int64_t ws_bytes,
                        hipStream_t s);
int64_t subgraph_workspace(int64_t n, int64_t m, int64_t nnz);
int subgraph_count(const int32_t *row_ptr, const int32_t *col, int64_t n, const int64_t *idx,
                   int64_t m, int64_t nnz, int32_t *out_row_ptr, void *ws, int64_t ws_bytes,
                   int64_t *out_nnz_host, uint32_t *status_host, hipStream_t s);
int subgraph_fill(const int32_t *row_ptr, const int32_t *col, const double *val, int64_t n,
                  const int64_t *idx, int64_t m, int64_t nnz, const int32_t *out_row_ptr,
                  int32_t *out_col, double *out_val, void *ws, int64_t ws_bytes, hipStream_t s);
int set_tuning(const char *key, int64_t value);
int64_t get_tuning(const char *key);
int timing_enable(int on);
int timing_collect(float *light_ms, float *hub_ms, int64_t capacity, int64_t *n_host);
int timing_collect_ex(float *light_ms, float *hub_ms, float *span_ms, int32_t *kernel,
                      int64_t capacity, int64_t *n_host);
int coo_to_csr_cpu(const int64_t *rows, const int64_t *cols, const float *vals, int64_t nnz,
                   int64_t n_rows, int64_t n_cols, int32_t *row_ptr, int32_t *col_idx,
                   float *val_out, uint32_t *status_host);
int spmm_cpu(const int32_t *row_ptr, const int32_t *col_idx, const float *val, int64_t row_begin,
             int64_t row_end, const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
             int32_t n_threads, bool accum);
int64_t propagate_cpu_workspace(int64_t n_rows, int64_t F, int32_t K);
int propagate_cpu(const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                  int64_t n_rows, const float *X0, int64_t ldx, float *out, int64_t ldo, int64_t F,
                  int32_t K, void *workspace, int64_t workspace_bytes, int32_t n_threads);
const char *linear_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C, const float *X);
const char *linear_backward_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                        const float *X);
int launch_linear_f32(const float *X, int64_t ldx, const float *W, const float *b, float *Y,
                      int64_t ldy, int64_t M, int64_t K, int64_t C, hipStream_t stream);
// the x_dtype of every 16-bit classifier entry (linear16.hip, xent16.hip, eval16.hip)
inline bool dtype_ok(int32_t x_dtype) {
    return x_dtype == SGC_DTYPE_BF16 || x_dtype == SGC_DTYPE_F16;
}
const char *linear_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C, const void *X,
                                   int32_t x_dtype);
int launch_linear_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                      float *Y, int64_t ldy, int64_t M, int64_t K, int64_t C, hipStream_t stream);
const char *linear_backward_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                            const void *X, int32_t x_dtype);
int64_t linear_backward_x16_workspace_bytes(int64_t M, int64_t K, int64_t C);
int linear_backward_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *dY, int64_t ldd,
                        int64_t M, int64_t K, int64_t C, float *dW, float *db, void *ws,
                        int64_t ws_bytes, hipStream_t s);
// linear16.hip: launch B of the fused 16-bit step (the plain kernel) and its row ranges
int dw_cols_x16_ranges(int64_t M);
hipError_t launch_dw_cols_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *G, int ldg,
                              int M, int K, int C, float *slab, float *db_slab, hipStream_t s);
// xent16.hip: the fused step and the training loops on 16-bit features
const char *linear_xent_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                        const void *X, int32_t x_dtype);
int64_t linear_xent_x16_workspace_bytes(int64_t M, int64_t K, int64_t C);
int linear_xent_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, float *loss, float *dW,
                    float *db, void *ws, int64_t ws_bytes, hipStream_t s);
int xent_x16_closure_check(const char *what, const void *X, int32_t x_dtype, int64_t ldx, int64_t M,
                           int64_t K, int64_t C);
int xent_x16_closure(const int64_t *stop, const void *X, int32_t x_dtype, int64_t ldx,
                     const float *W, const float *b, const int64_t *labels, int64_t M, int64_t K,
                     int64_t C, float *loss, float *dW, float *db, void *ws, hipStream_t s);
int64_t train_adam_x16_workspace(int64_t M, int64_t K, int64_t C);
int train_adam_x16(const void *X, int32_t x_dtype, int64_t ldx, float *W, float *b,
                   const int64_t *labels, int64_t M, int64_t K, int64_t C, float *mW, float *vW,
                   float *mb, float *vb, int64_t step0, int32_t epochs, double lr, double beta1,
                   double beta2, double eps, double weight_decay, float *loss_trace, void *ws,
                   int64_t ws_bytes, hipStream_t s);
int64_t train_lbfgs_x16_workspace(int64_t M, int64_t K, int64_t C);
int train_lbfgs_x16(const void *X, int32_t x_dtype, int64_t ldx, float *W, float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, void *state,
                    int32_t steps, double lr, int32_t max_iter, int32_t max_eval, double tol_grad,
                    double tol_change, float *loss_trace, int64_t *status_trace, void *ws,
                    int64_t ws_bytes, hipStream_t s);
// eval.hip / eval16.hip: device-resident evaluation (sgc_linear_eval_f32 / _x16).
// Shared by the two units: the workspace (loss partials, counter tables, the
// predictions the counts read when the caller passes no `pred`), the pointer
// rules, and the counting and finishing launches behind either forward.
struct EvalParts {
    double *loss_part;
    int32_t *count_part;
    int64_t *pred;
};
int64_t eval_workspace_bytes(int64_t M, int64_t C, int64_t n_loss);
EvalParts eval_carve(void *ws, int64_t M, int64_t C, int64_t n_loss);
int eval_check_outputs(const char *what, const int64_t *labels, const int64_t *pred,
                       const int64_t *confusion, const int64_t *counts, const float *loss);
int eval_count_finish(const int64_t *labels, const int64_t *pred, int64_t M, int64_t C,
                      const EvalParts &o, int n_loss, int64_t *confusion, int64_t *counts,
                      float *loss, hipStream_t s);
const char *linear_eval_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C, const float *X);
int64_t linear_eval_workspace_bytes(int64_t M, int64_t K, int64_t C);
int linear_eval_f32(const float *X, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, int64_t *pred,
                    int64_t *confusion, int64_t *counts, float *loss, void *ws, int64_t ws_bytes,
                    hipStream_t s);
const char *linear_eval_x16_kernel_name(int64_t M, int64_t K, int64_t ldx, int64_t C,
                                        const void *X, int32_t x_dtype);
int64_t linear_eval_x16_workspace_bytes(int64_t M, int64_t K, int64_t C);
int linear_eval_x16(const void *X, int32_t x_dtype, int64_t ldx, const float *W, const float *b,
                    const int64_t *labels, int64_t M, int64_t K, int64_t C, int64_t *pred,
                    int64_t *confusion, int64_t *counts, float *loss, void *ws, int64_t ws_bytes,
                    hipStream_t s);
int64_t plan_sorted_workspace(int64_t n_rows);
int64_t colsplit_workspace(int64_t n_rows, int32_t groups);
int mgpu_init(int ndev, const int *devices);
int mgpu_finalize();
int mgpu_attach(const int32_t *row_ptr, const int32_t *col_idx, const float *val, int64_t n,
                int64_t nnz, hipStream_t stream, int64_t *handle);
int mgpu_detach(int64_t handle);
int mgpu_propagate(int64_t handle, const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t F,
                   int32_t K, hipStream_t stream);
int64_t lbfgs_workspace(int64_t n, int32_t history_size);
int lbfgs_init(void *state, int64_t bytes, int64_t n, int32_t history_size, hipStream_t s);
// (begin_step and read_status serve both engines' states; `what` names the entry)
int lbfgs_begin_step(const char *what, void *state, hipStream_t s);
int lbfgs_iterate(void *state, int32_t n_tensors, float *const *params, const float *const *grads,
                  const int64_t *numels, const float *loss, double lr, int32_t max_iter,
                  int32_t max_eval, double tol_grad, double tol_change, hipStream_t s);
int lbfgs_read_status(const char *what, const void *state, int64_t *out_host, hipStream_t s);
int64_t train_lbfgs_workspace(int64_t M, int64_t K, int64_t C);
int train_lbfgs(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels, int64_t M,
                int64_t K, int64_t C, void *state, int32_t steps, double lr, int32_t max_iter,
                int32_t max_eval, double tol_grad, double tol_change, float *loss_trace,
                int64_t *status_trace, void *ws, int64_t ws_bytes, hipStream_t s);
// lbfgs_wide.hip: the iteration in Gram form over the whole machine
hipError_t warm_lbfgs_wide(hipStream_t);
int64_t lbfgs_wide_workspace(int64_t n, int32_t history_size);
int lbfgs_wide_init(void *state, int64_t bytes, int64_t n, int32_t history_size, hipStream_t s);
int lbfgs_wide_iterate(void *state, int32_t n_tensors, float *const *params,
                       const float *const *grads, const int64_t *numels, const float *loss,
                       double lr, int32_t max_iter, int32_t max_eval, double tol_grad,
                       double tol_change, hipStream_t s);
int lbfgs_wide_sync_gram(void *state, hipStream_t s);
int lbfgs_wide_l2(void *state, const float *W, float *gW, int64_t numel, double l2, float *loss,
                  hipStream_t s);
int64_t train_lbfgs_wide_workspace(int64_t M, int64_t K, int64_t C);
int train_lbfgs_wide(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                     int64_t M, int64_t K, int64_t C, void *state, int32_t steps, double lr,
                     int32_t max_iter, int32_t max_eval, double tol_grad, double tol_change,
                     double l2, float *loss_trace, int64_t *status_trace, void *ws,
                     int64_t ws_bytes, hipStream_t s);
int adam_set_tuning(int64_t value);
int adam_sweep_set_form(int64_t value);
int64_t adam_small_max_rows();
int adam_step(int32_t n_tensors, float *const *params, const float *const *grads,
              float *const *exp_avgs, float *const *exp_avg_sqs, const int64_t *numels,
              int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
              hipStream_t s);
int64_t train_adam_workspace(int64_t M, int64_t K, int64_t C);
int train_adam(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels, int64_t M,
               int64_t K, int64_t C, float *mW, float *vW, float *mb, float *vb, int64_t step0,
               int32_t epochs, double lr, double beta1, double beta2, double eps,
               double weight_decay, float *loss_trace, void *ws, int64_t ws_bytes, hipStream_t s);
int64_t train_adam_sweep_workspace(int64_t B, int64_t M, int64_t K, int64_t C);
int train_adam_sweep(const float *X, int64_t ldx, float *W, float *b, const int64_t *labels,
                     int64_t B, int64_t M, int64_t K, int64_t C, float *mW, float *vW, float *mb,
                     float *vb, int64_t step0, int32_t epochs, double lr, double beta1,
                     double beta2, double eps, const float *wd_dev, float *loss_trace, void *ws,
                     int64_t ws_bytes, hipStream_t s);
int linear_eval_sweep_f32(const float *X, int64_t ldx, const float *W, const float *b,
                          const int64_t *labels, int64_t B, int64_t M, int64_t K, int64_t C,
                          int64_t *pred, int64_t *confusion, int64_t *counts, float *loss, void *ws,
                          int64_t ws_bytes, hipStream_t s);


}  // namespace sgc
