/*
 * mgn_hip_slice.h -- the physics (slice) attention of the Transolver processor (model.type "transolver"): the Gumbel-softmax slice
 * weights of every (node, head) row, the reductions over all nodes into heads x slice_num tokens, the broadcast back to the rows
 * and the per-row backward.
 *
 * Same conventions as mgn_hip_ext.h / mgn_hip_mtp.h: raw DEVICE pointers, plain sizes and a hipStream_t (passed as void*); 0 on
 * success, 1 when the arguments are refused (before any launch; the text names the entry point), 2 on a HIP error, with the text
 * in mgn_attn_last_error() (every entry point here is defined in csrc/mgn_slice.inc, included by csrc/mgn_attn.hip); nothing is
 * allocated, no state is kept, every launch is asynchronous on `stream`.  No structs: scalar and pointer arguments only, so
 * mgn_version() stays 136.  No atomics anywhere: every sum over nodes runs in a fixed order (workgroup partials in the caller's
 * workspace, summed in index order by a finishing launch), so results are bit-identical from run to run.
 *
 * All data is fp32.  N rows (nodes), H heads, G slices, C = hidden / heads channels per head.  Row matrices are N-major with a
 * leading dimension in floats: x_mid[n * ldx + h * C + c];  w is [N, H, G] dense;  tokens are [H, G, C] dense.
 * Supported: 1 <= G <= 64, 1 <= C <= 64, 1 <= H <= 65535, 0 <= layer < 4096, N * H < 2^44.  N == 0 returns 0 without a launch
 * (the reductions then write zeros).
 *
 * Noise stream.  u[n, h, g] = (word >> 8) * 2^-24 in [0, 1), word = output word (g & 1) of Philox4x32-10 with
 *   key     = (seed low 32 bits, seed high 32 bits)
 *   counter = (row low 32 bits,  (g >> 1) | layer << 8 | (row >> 32) << 20,  step low 32 bits,  (step >> 32) ^ 0x534c4943)
 * where row = n * H + h.  u depends on (seed, step, layer, n, h, g) only, never on the launch geometry.  `step` is read from a
 * DEVICE int64 by the kernel (null = 0): a captured replay that advances the scalar on the stream draws new noise.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   graphphysics/models/transolver.py   gumbel_softmax, Physics_Attention_1D_Eidetic.forward (the [B, H, N, C] einsums there)
 */
#ifndef MGN_HIP_SLICE_H
#define MGN_HIP_SLICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Rows that ONE pass of the grid covers before its workgroups loop on:  launch 2 = mgn_slice_weights_fwd (counted in (row, head)
 * pairs), 3 = mgn_slice_aggregate (nodes, at H = 1: its workgroups are shared out over the heads, 1 / H of this with H heads),
 * 4 = mgn_slice_expand (nodes), 5 = mgn_slice_rows_bwd (nodes, per head).  0 for any
 * other launch number or G outside 1..64.  (Tests place a row count just above twice this.) */
int64_t mgn_slice_pass_rows(int launch, int G);

/* ------------------------------------------------------------- 1: the uniforms
 * u[N, H, G] of the stream above: what launch 2 draws when its `u` is null. */
int mgn_slice_uniforms(uint64_t seed, const int64_t* step, int layer, int64_t N, int H, int G, float* u, void* stream);

/* ------------------------------------------------------------- 2: slice weights
 * Per (row, head), x = x_mid[n, h*C : (h+1)*C]:
 *   h1[g]  = GELU(W1[g, :] . x + b1[g])                       W1 [G, C], b1 [G]          (proj_temperature.0)
 *   t2     = w2 . h1 + b2                                     w2 [G], b2 [1]             (proj_temperature.2)
 *   tpre   = GELU(t2) + bias[h],   t = max(tpre, 0.01)        bias [H]
 *   a[g]   = Ws[g, :] . x + bs[g]                             Ws [G, C], bs [G]          (in_project_slice)
 *   gum[g] = -log(-log(u + 1e-8) + 1e-8)    in fp32, precise logf
 *   w[g]   = softmax_g((y[g] - max_k y[k]) / t),  y = a + gum    (= softmax_g(y / t); the row maximum goes before the division)
 * u [N, H, G] or null (then drawn from the stream (seed, *step, layer)).  GELU is the exact erf form.
 * Writes w [N, H, G] and rowsc [N * H, 2] = {t2, tpre} (the pre-clamp temperature and the pre-activation in front of it). */
int mgn_slice_weights_fwd(const float* x_mid, int64_t ldx, const float* Ws, const float* bs, const float* W1, const float* b1,
                          const float* w2, const float* b2, const float* bias, const float* u, uint64_t seed, const int64_t* step,
                          int layer, int64_t N, int H, int G, int C, float* w, float* rowsc, void* stream);

/* ------------------------------------------------------------- 3: reduction over the nodes
 * S[h, g, c] = sum_n w[n, h, g] * x[n * ldx + h * C + c]      S [H, G, C]
 * norm[h, g] = sum_n w[n, h, g]                               norm [H, G], optional (null: not written)
 * Every workgroup sums a contiguous range of nodes in ascending order into the workspace; a second launch adds the partials in
 * index order.  The forward calls it with x_mid; the backward with dOut_x (giving d out_token), and with H = 1 over the N * H
 * (row, head) pairs for the weight gradients dWs = da^T x, dW1 = dh1^T x (norm then holds dbs, db1). */
size_t mgn_slice_aggregate_workspace_bytes(int64_t N, int H, int G, int C);
int mgn_slice_aggregate(const float* w, const float* x, int64_t ldx, int64_t N, int H, int G, int C, float* S, float* norm, void* ws,
                        size_t ws_bytes, void* stream);

/* ------------------------------------------------------------- 4: broadcast back to the rows
 * out[n * ldo + h * C + c] = sum_g w[n, h, g] * tok[h, g, c]  (g ascending) */
int mgn_slice_expand(const float* w, const float* tok, int64_t N, int H, int G, int C, float* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------- 5: per-row backward
 * Inputs: dOut [N, lddo] (the gradient of launch 4's output), tok = out_token [H, G, C], dS [H, G, C] and dnorm [H, G] (the
 * gradients of launch 3's outputs), x_mid, w and rowsc of the forward, the small weights, and the forward's noise source
 * (u, or null and seed / step / layer: the logits a + gum are formed again, bit for bit, never stored).
 *   dw[g]  = <dOut[n, h], tok[h, g]> + <x, dS[h, g]> + dnorm[h, g]
 *   dz[g]  = w[g] * (dw[g] - sum_k w[k] dw[k])
 *   da[g]  = dz[g] / t                                                            da  [N * H, G]
 *   dtpre  = -sum_g dz[g] (y[g] - max_k y[k]) / t^2  where tpre >= 0.01, else 0   (sum_g dz[g] = 0: the constant changes nothing
 *            but the rounding -- the sum no longer cancels at the size of y)
 *   dt2    = dtpre * GELU'(t2)                                                    dt2 [N * H]
 *   dh1[g] = dt2 * w2[g] * GELU'(W1[g, :] . x + b1[g])   (gradient of the PRE-activation)   dh1 [N * H, G]
 *   dx[n * lddx + h*C + c] = sum_g (w[g] dS[h, g, c] + Ws[g, c] da[g] + W1[g, c] dh1[g])      the complete d x_mid
 * and the three parameter gradients that need nothing but these row values, in fixed order through the workspace:
 *   dw2[g] = sum_rows dt2 * h1[g]   [G],   db2 = sum_rows dt2   [1],   dbias[h] = sum_n dtpre   [H]
 * The others come from launch 3 over the (row, head) pairs: dWs, dbs from da;  dW1, db1 from dh1. */
size_t mgn_slice_rows_bwd_workspace_bytes(int64_t N, int H, int G);
int mgn_slice_rows_bwd(const float* dOut, int64_t lddo, const float* tok, const float* dS, const float* dnorm, const float* x_mid,
                       int64_t ldx, const float* w, const float* rowsc, const float* Ws, const float* bs, const float* W1,
                       const float* b1, const float* w2, const float* u, uint64_t seed, const int64_t* step, int layer, int64_t N,
                       int H, int G, int C, float* dx, int64_t lddx, float* da, float* dh1, float* dt2, float* dw2, float* db2,
                       float* dbias, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MGN_HIP_SLICE_H */
