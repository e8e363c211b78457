/*
 * mgn_hip_ext.h -- entry points added after ABI 136 of mgn_hip.h.
 *
 * Same conventions as mgn_hip.h: raw DEVICE pointers, plain sizes and a hipStream_t (passed as void*); 0 on success,
 * non-zero on error with the text in the defining unit's error channel (every entry point here is defined in
 * csrc/mgn_prep.hip or a file it includes: mgn_prep_last_error()); nothing is allocated, no state is kept, every launch
 * is asynchronous on `stream`.  No structs: scalar and pointer arguments only, so mgn_version() stays 136 and a binding
 * of mgn_hip.h alone keeps working.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   mgn_rollout_tail   the statements after the model of LightningModule._make_prediction and validation_step
 *                        graphphysics/training/lightning_module.py:387-401,439-455
 */
#ifndef MGN_HIP_EXT_H
#define MGN_HIP_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------- validation rollout: the tail of one frame
 * Two launches.  The first writes
 *   pred[N, O]  exactly mgn_sim_post(..., mask_truth = 1): x[:, out_start:+O] + (net_out * std + mean) of the output
 *               normaliser, the ground truth y[:, 0:O] where the node type (compared as a float: 0.5 is neither) is not
 *               NORMAL / OUTFLOW -- bit-identical, the two share one device function;
 *   prev[N, O]  (optional, may be null) pred - x[:, out_start:+O], taken after the re-imposition: what the reference feeds
 *               back into x[:, previous_data_start:previous_data_end] (lightning_module.py:383-386,400-401);
 * and, when `metrics` is not null, per-block partial sums into part (mgn_rollout_tail_scratch_floats() floats).  The second
 * launch (only with `metrics`) adds them in fp64 in a fixed order and stores row *slot of metrics[cap][4]:
 *   S_all   = sum over all rows and columns of (pred - y)^2        (val_1step_rmse, val_all_rollout_rmse: :452-455,:467-474)
 *   S_loss  = the same sum over the rows whose type is one of loss_types[0..n_loss_types)   (val_loss: :443-449)
 *   n_loss  = the number of such rows;  N
 * if 0 <= *slot < cap, and then *slot += 1 whether it stored or not: the table is never overrun, and the host, which reads
 * table and counter once after the last frame, sees *slot > cap.  The counter is a DEVICE int so that one captured graph
 * serves every frame.  `loss_types` is a HOST array of 1..4 codes.  N == 0 stores a zero row.  Deterministic: no atomics.
 * Returns 1 before any launch if O is outside 1..32, if y, pred or part is null, if metrics is given without 1..4 loss types,
 * a slot counter and cap >= 1, or if the column windows lie outside x / y. */
int mgn_rollout_tail_scratch_floats(void);
int mgn_rollout_tail(const float* x, int x_w, int out_start, int type_idx, const float* y, int y_w, const float* net_out, int O,
                     const float* acc_sum, const float* acc_sumsq, const float* acc_count, float std_eps,
                     const float* loss_types, int n_loss_types, int64_t N, float* pred, float* prev, float* part,
                     double* metrics, int* slot, int cap, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MGN_HIP_EXT_H */
