// The tail of one validation-rollout frame, included by mgn_prep.hip (sim_post_value, mse_w, SIM_MAXW and the error channel
// come from there); declared in include/mgn_hip_ext.h.
//
// The reference's validation loop (training/lightning_module.py:375-492) does per frame, after the model: build_outputs, the
// re-imposition of the ground truth, `predicted_outputs - current_output` for the previous-data columns, the masked L2 of the
// validation loss, the squared error of the RMSE metrics, and two `.cpu()` copies.  Here that is two launches and no copy:
//
//   k_rollout_tail   RT_PART blocks x 256 threads, grid-stride over the N x O elements.  Writes pred (sim_post_value, the
//                    arithmetic of k_sim_post with mask_truth = 1) and prev = pred - x[:, out_start + col]; accumulates per thread
//                    (pred - y)^2 over all rows, the same over the rows whose type is one of the loss types, and the number of
//                    such rows (counted at column 0); reduces by wave64 shuffles, then through LDS across the block's four waves,
//                    and writes three floats per block.
//   k_rollout_final  one block: the RT_PART partials summed in fp64 in a fixed order, stored as row *slot of the metrics table
//                    {S_all, S_loss, n_loss, N} if *slot < cap, and *slot += 1 in any case.
//
// The row index lives on the DEVICE so that one captured graph serves every frame of every trajectory; a table that is too
// small loses rows but is never overrun, and the host sees *slot > cap afterwards.  No atomics, fixed orders everywhere: the
// same bits on every run, launched eagerly or replayed.
#include "mgn_hip_ext.h"

#define RT_PART 256  // blocks of the row kernel = partial triples

__global__ void __launch_bounds__(256) k_rollout_tail(const float* __restrict__ x, int x_w, int out_start, int type_idx,
                                                      const float* __restrict__ y, int y_w, const float* __restrict__ net_out, int O,
                                                      const float* __restrict__ acc_sum, const float* __restrict__ acc_sumsq,
                                                      const float* __restrict__ acc_count, float std_eps, float t0, float t1, float t2,
                                                      float t3, int want_metrics, long N, float* __restrict__ pred,
                                                      float* __restrict__ prev, float* __restrict__ part) {
  __shared__ float s[3][4];
  float a = 0.f, b = 0.f, c = 0.f;
  const long total = N * O;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)RT_PART * 256) {
    const float p = sim_post_value(x, x_w, out_start, type_idx, y, y_w, net_out, O, acc_sum, acc_sumsq, acc_count, std_eps, 1, i);
    const long row = i / O;
    const int col = (int)(i % O);
    pred[i] = p;
    if (prev != nullptr) prev[i] = p - x[row * x_w + out_start + col];  // after the re-imposition, as the reference subtracts
    if (want_metrics) {
      const float d = p - y[row * y_w + col];
      a = fmaf(d, d, a);
      if (mse_w(x[row * x_w + type_idx], t0, t1, t2, t3) != 0.f) {
        b = fmaf(d, d, b);
        if (col == 0) c += 1.f;
      }
    }
  }
  if (!want_metrics) return;
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
    c += __shfl_down(c, off, 64);
  }
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) s[0][wave] = a, s[1][wave] = b, s[2][wave] = c;
  __syncthreads();
  if (threadIdx.x < 3) {
    const float* v = s[threadIdx.x];
    part[3 * blockIdx.x + threadIdx.x] = ((v[0] + v[1]) + v[2]) + v[3];
  }
}

__global__ void __launch_bounds__(256) k_rollout_final(const float* __restrict__ part, long N, double* __restrict__ metrics,
                                                       int* __restrict__ slot, int cap) {
  __shared__ double s[3][4];
  double v[3];
  for (int k = 0; k < 3; ++k) v[k] = (double)part[3 * threadIdx.x + k];  // RT_PART == the block size: one triple per thread
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 3; ++k) v[k] += __shfl_down(v[k], off, 64);
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0)
    for (int k = 0; k < 3; ++k) s[k][wave] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int at = *slot;
    if (at >= 0 && at < cap) {
      double* m = metrics + 4 * (long)at;
      for (int k = 0; k < 3; ++k) m[k] = ((s[k][0] + s[k][1]) + s[k][2]) + s[k][3];
      m[3] = (double)N;
    }
    if (at < 0x7fffffff) *slot = at + 1;
  }
}

extern "C" int mgn_rollout_tail_scratch_floats(void) { return 3 * RT_PART; }

extern "C" int mgn_rollout_tail(const float* x, int x_w, int out_start, int type_idx, const float* y, int y_w, const float* net_out,
                                int O, const float* acc_sum, const float* acc_sumsq, const float* acc_count, float std_eps,
                                const float* loss_types, int n_loss_types, int64_t N, float* pred, float* prev, float* part,
                                double* metrics, int* slot, int cap, void* stream) {
  static_assert(RT_PART == 256, "k_rollout_final reads one partial triple per thread of its one block");
  if (O < 1 || O > SIM_MAXW) return fail(1, "mgn_rollout_tail: output width outside 1..32");
  if (y == nullptr || pred == nullptr || part == nullptr) return fail(1, "mgn_rollout_tail: y, pred and part must not be null");
  if (x == nullptr || net_out == nullptr || acc_sum == nullptr || acc_sumsq == nullptr || acc_count == nullptr || N < 0 ||
      out_start < 0 || out_start + O > x_w || type_idx < 0 || type_idx >= x_w || y_w < O)
    return fail(1, "mgn_rollout_tail: bad arguments");
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  if (metrics != nullptr) {
    if (n_loss_types < 1 || n_loss_types > 4 || loss_types == nullptr) return fail(1, "mgn_rollout_tail: 1..4 loss node types");
    if (slot == nullptr || cap < 1) return fail(1, "mgn_rollout_tail: metrics need a slot counter and a capacity >= 1");
    for (int k = 0; k < 4; ++k) t[k] = loss_types[k < n_loss_types ? k : 0];
  }
  hipStream_t s = (hipStream_t)stream;
  const int want = metrics != nullptr;
  hipLaunchKernelGGL(k_rollout_tail, dim3(RT_PART), dim3(256), 0, s, x, x_w, out_start, type_idx, y, y_w, net_out, O, acc_sum, acc_sumsq,
                     acc_count, std_eps, t[0], t[1], t[2], t[3], want, (long)N, pred, prev, part);
  if (want) hipLaunchKernelGGL(k_rollout_final, dim3(1), dim3(256), 0, s, (const float*)part, (long)N, metrics, slot, cap);
  return check_launch("mgn_rollout_tail");
}
