/*
 * mgn_hip_mtp.h -- the spatial multi-token-prediction branch of the training step (training.use_spatial_mtp): dense attention
 * inside the row segments ("stars") of one packed matrix, the packing around it and the loss tail.
 *
 * Same conventions as mgn_hip_ext.h: raw DEVICE pointers, plain sizes and a hipStream_t (passed as void*); 0 on success, 1 when
 * the arguments are refused (before any launch), 2 on a HIP error, with the text in mgn_attn_last_error() (every entry point here
 * is defined in csrc/mgn_starattn.inc, included by csrc/mgn_attn.hip); nothing is allocated, no state is kept, every launch is
 * asynchronous on `stream`.  No structs: scalar and pointer arguments only, so mgn_version() stays 136.  No atomics anywhere:
 * every sum runs in a fixed order, results are bit-identical from run to run.
 *
 * Star b of a packed matrix owns rows [off[b], off[b+1]): its first row is the centre node, the others its kept 1-hop
 * neighbours.  off[B+1] is int32, ascending, off[0] = 0, off[B] = R.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   graphphysics/models/spatial_mtp_1hop.py   SpatialMTP1Hop.forward / _cap_neighbors (padded [B, 1 + max_deg, d] there)
 */
#ifndef MGN_HIP_MTP_H
#define MGN_HIP_MTP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------- star offsets
 * One launch of one workgroup.  deg_b = rowptr[centers[b] + 1] - rowptr[centers[b]], cut to max_neighbors when that is > 0;
 * off[0] = 0, off[b + 1] = off[b] + 1 + deg_b;  meta = {R = off[B], flags};  stats = {pairs = R - B, max_b deg_b} as floats.
 * flags bit 0: a centre outside [0, N) (it counts as a star without neighbours), bit 1: R above INT32_MAX / 384 (off is then
 * not to be used).  Sized for a training step's few hundred to few thousand centres: ONE workgroup scans them in chunks of 256, so
 * the time grows linearly with B (correct up to the row limit, not fast there).  Returns 1 if a pointer is null, N < 0, B < 0 or
 * B > INT32_MAX / 384;  B == 0 writes meta and stats of zeros in the same launch. */
int mgn_star_offsets(const int32_t* rowptr, const int32_t* centers, int64_t N, int64_t B, int max_neighbors, int32_t* off,
                     int32_t* meta, float* stats, void* stream);

/* ------------------------------------------------------------- neighbour cap
 * keep[R - B]: for star b the positions (within the centre's row of the CSR) of its kept neighbours, at keep[off[b] - b ...].
 * A centre with c <= max_neighbors neighbours keeps 0 .. c-1 in order.  Otherwise the max_neighbors positions with the smallest
 * of c 64-bit keys, key_j = the two words of Philox4x32-10 with key (seed low, seed high) and counter (j, b, step, 0x4d5450),
 * ties broken by j: a uniform draw without replacement, stored in ascending key order.  Returns 1 if a pointer is null or
 * max_neighbors < 1;  B == 0 returns 0 without a launch. */
int mgn_star_cap(const int32_t* rowptr, const int32_t* centers, const int32_t* off, int64_t N, int64_t B, int max_neighbors,
                 uint64_t seed, uint32_t step, int32_t* keep, void* stream);

/* ------------------------------------------------------------- pack
 * One launch.  Row r = off[b] + t of star b is node centers[b] (t = 0, read from H) or node nbr[rowptr[centers[b]] + p]
 * (t >= 1, read from H_neigh) with p = t - 1, or p = keep[r - b - 1] when keep is given.
 *   row_node[R], row_star[R]     node and star of a row
 *   row_key[R]                   row_node, plus key_offset on centre rows: the grouping key of the backward
 *   nb_rows[R - B]               the packed row of every neighbour row, in order
 *   nb_ptr[R + 1]                nb_ptr[r] = number of neighbour rows before row r (the transpose of nb_rows as a CSR)
 *   X0[R, d]                     the gathered rows;  inv[R] = 1 / (||x|| / sqrt(d) + 1e-8)
 *   X[R, d]                      scale * x * inv (graphphysics/models/layers.py:104-129: eps outside the root)
 * A node index outside [0, N) gives a row of zeros and row_node = -1.  d in {16, 32, 64, 128}.  R == 0 or B == 0 returns 0
 * without a launch. */
int mgn_star_pack(const int32_t* rowptr, const int32_t* nbr, const int32_t* centers, const int32_t* off, const int32_t* keep,
                  const float* H, const float* H_neigh, const float* scale, int64_t N, int64_t B, int64_t R, int d,
                  int64_t key_offset, int32_t* row_node, int32_t* row_star, int64_t* row_key, int32_t* nb_rows, int32_t* nb_ptr,
                  float* X0, float* X, float* inv, void* stream);

/* ------------------------------------------------------------- attention inside the stars
 * qkv[R, 3d] is one in-projection's output in nn.MultiheadAttention's layout: q, k, v are the column slabs [0, d), [d, 2d),
 * [2d, 3d) at pitch 3d, head h owns columns [h * dh, (h + 1) * dh) of each, dh = d / heads.  For row i of star b and head h:
 *   score_ij = q_i . k_j / sqrt(dh) over the rows j of the star,  P = softmax_j(score),  y[i] = sum_j P_ij v_j      y[R, d]
 *   lse[i, h] = log sum_j exp(score_ij)                                                                         lse[R, heads]
 * One workgroup per star; keys and values pass through LDS in tiles of mgn_star_attn_tile_rows() rows with a running maximum and
 * sum, so a segment of any length >= 1 is valid.  The backward returns dqkv[R, 3d] from dy[R, d], qkv, y and lse.
 * d in {16, 32, 64, 128}, heads in {1, 2, 4, 8, 16} dividing d.  R == 0 or B == 0 returns 0 without a launch.  Returns 1 for
 * d or heads outside those sets, a null pointer, or R above INT32_MAX / (3 * 128). */
int mgn_star_attn_tile_rows(void);
int mgn_star_attn_fwd(const float* qkv, const int32_t* off, int64_t R, int64_t B, int d, int heads, float* y, float* lse,
                      void* stream);
int mgn_star_attn_bwd(const float* dy, const float* qkv, const float* y, const float* lse, const int32_t* off, int64_t R,
                      int64_t B, int d, int heads, float* dqkv, void* stream);

/* ------------------------------------------------------------- loss tail
 * yhat[T, O] holds the decoder's output on the neighbour rows only (T = R - B, the order of nb_rows).  err_t = the mean over the
 * O columns of (yhat[t] - target[row_node of t])^2 in fp32, summed in fp64 in a fixed order:
 *   reduction 0 ("mean_per_center")   loss = mean_b (sum of err_t over star b) / max(deg_b, 1)
 *   reduction 1 ("mean")              loss = mean_t err_t
 * out = {loss, mean_t err_t};  dyhat[T, O] = d loss / d yhat.  One launch of one workgroup, one thread per star walking its rows in
 * order: sized for a training step's few hundred to few thousand stars of mesh degree; a far larger B or a hub's star is summed
 * correctly but serially.  O in 1..32, T >= 1, B >= 1. */
int mgn_star_loss(const float* yhat, const float* target, const int32_t* row_node, const int32_t* off, int64_t N, int64_t B,
                  int64_t R, int O, int reduction, float* out, float* dyhat, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MGN_HIP_MTP_H */
