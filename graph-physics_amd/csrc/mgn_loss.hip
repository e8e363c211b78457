// MI355X (gfx950) kernels of a training config's "loss" section (graphphysics/utils/loss.py on top of
// utils/vectorial_operators.py): the three pointwise losses on the normalised output and the five physics losses on the nodal
// spatial gradient G [N, F, DX] of the physical fields.  G is a fixed sparse linear operator on an [N, F] field, so the work splits:
//   * geometry, once per mesh (mgn_loss_fd_geometry / mgn_loss_ls_geometry): coefficients computed in fp64, stored as fp32;
//   * per step (mgn_loss_fwd / mgn_loss_bwd): one gather pass per node that holds G_out[n] and G_tgt[n] in registers, evaluates every
//     configured term for the node, masks, block-reduces, and leaves the node's dL/dG and direct dL/dU for the backward -- which is
//     the TRANSPOSED gather over the same index (c_mn = -c_nm for finite differences; the element's own corner list for least
//     squares).  No float atomics anywhere: every sum has a fixed order, results are bit-identical run to run.  No host
//     synchronisation, no data-dependent shape: the selected-row count is a device scalar.
// Fifth translation unit of libmgn_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "mgn_hip.h"

#include "mgn_host.inc"  // g_err, fail, check_launch
extern "C" const char* mgn_loss_last_error(void) { return g_err; }

#define LF MGN_LOSS_MAX_F
#define LD MGN_LOSS_MAX_D
#define LOSS_PART 1024   // blocks of the node pass = rows of the partial table

// ===================================================================== geometry: finite differences
// per node n over its row of the de-duplicated symmetric neighbour CSR (no self entries; self_loop[n] != 0 marks a pair (n, n)):
//   dx = pos[m] - pos[n], w = 1 / (|dx|^2 + 1e-8), c_nm = dx * w / (|dx|^2 + 1e-8), inv[n] = 1 / (sum_m w + [self] 2e8 + 1e-8)
// (vectorial_operators.py:95-127: a pair adds the same product to both of its ends, so a self pair adds 2 w = 2e8 to the weight sum
// and, dx being 0, nothing to the numerator)
__global__ void __launch_bounds__(256) k_fd_geom(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const uint8_t* __restrict__ self_loop, const float* __restrict__ pos, int DX, long N,
                                                 float* __restrict__ coef, float* __restrict__ inv) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double pn[LD];
  for (int d = 0; d < DX; ++d) pn[d] = (double)pos[n * DX + d];
  double wsum = (self_loop != nullptr && self_loop[n]) ? 2.0 / 1e-8 : 0.0;
  for (int64_t k = rowptr[n]; k < rowptr[n + 1]; ++k) {
    const long m = col[k];
    double dx[LD], r2 = 0.0;
    for (int d = 0; d < DX; ++d) {
      dx[d] = (double)pos[m * DX + d] - pn[d];
      r2 += dx[d] * dx[d];
    }
    const double w = 1.0 / (r2 + 1e-8);
    wsum += w;
    for (int d = 0; d < DX; ++d) coef[k * DX + d] = (float)(dx[d] * w * w);
  }
  inv[n] = (float)(1.0 / (wsum + 1e-8));
}

// ===================================================================== geometry: least squares
// per element (K = S + 1 corners, S = 2 triangle / 3 tetrahedron): A = P[1:] - P[0] (S x DX); grad_e = lstsq(A, B)^T is linear in the
// corner values with C = pinv(A) (DX x S): corner s + 1 carries column s, corner 0 minus their sum.  Stored: cv[e, k, :] = C column * vol_e.
// S == DX: adjugate / determinant.  S = 2 in 3-D: Gram-Schmidt of the two edge vectors, then the 2 x 2 triangular solve in that
// basis (the minimum-norm solution).  Never the Gram matrix A A^T: it squares the condition number, and hull slivers reach 2.5e4.
// An element of zero measure contributes nothing -- and zero means zero to fp64 rounding: collinear corners off the axes, or a
// corner listed twice, leave a determinant (or a Gram-Schmidt remainder) of 1e-17 rather than 0, and C * vol of such an element is
// not small (C ~ 1 / det): it would be adj(A) / 6, as large as a sound element's coefficients.  So a measure under LS_FLAT of the
// product of the edge lengths counts as zero; distinct fp32 positions cannot make a sine that small except by being collinear.
#define LS_FLAT 1.5e-14   // ~ 64 fp64 epsilons
__global__ void __launch_bounds__(256) k_ls_elem_geom(const int32_t* __restrict__ elems, long M, int K, const float* __restrict__ pos, int DX,
                                                      float* __restrict__ cv, double* __restrict__ vol) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M) return;
  const int S = K - 1;
  double P[4][LD], A[3][LD], C[LD][3];   // C[d][s]
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < DX; ++d) P[k][d] = (double)pos[(long)elems[e * K + k] * DX + d];
  for (int s = 0; s < S; ++s)
    for (int d = 0; d < DX; ++d) A[s][d] = P[s + 1][d] - P[0][d];
  for (int d = 0; d < LD; ++d)
    for (int s = 0; s < 3; ++s) C[d][s] = 0.0;
  double v = 0.0;
  if (S == 2 && DX == 2) {
    const double det = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    const double len = sqrt((A[0][0] * A[0][0] + A[0][1] * A[0][1]) * (A[1][0] * A[1][0] + A[1][1] * A[1][1]));
    if (fabs(det) > LS_FLAT * len) {   // A^-1 = adj / det; C[d][s] = (A^-1)[d][s]
      v = 0.5 * fabs(det);
      C[0][0] = A[1][1] / det, C[0][1] = -A[0][1] / det;
      C[1][0] = -A[1][0] / det, C[1][1] = A[0][0] / det;
    }
  } else if (S == 3 && DX == 3) {
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
                 c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
    double len = 1.0;
    for (int s = 0; s < 3; ++s) len *= sqrt(A[s][0] * A[s][0] + A[s][1] * A[s][1] + A[s][2] * A[s][2]);
    if (fabs(det) > LS_FLAT * len) {   // (A^-1)[d][s] = cofactor[s][d] / det
      v = fabs(det) / 6.0;
      C[0][0] = c00 / det, C[1][0] = c01 / det, C[2][0] = c02 / det;
      C[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
      C[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
      C[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
      C[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
      C[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
      C[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    }
  } else {   // S == 2, DX == 3 (validated by the host): a0 = r00 q0, a1 = r01 q0 + r11 q1; pinv(A) = Q^T L^-1
    const double r00 = sqrt(A[0][0] * A[0][0] + A[0][1] * A[0][1] + A[0][2] * A[0][2]);
    if (r00 > 0.0) {
      double q0[3], q1[3], w[3];
      for (int d = 0; d < 3; ++d) q0[d] = A[0][d] / r00;
      const double r01 = q0[0] * A[1][0] + q0[1] * A[1][1] + q0[2] * A[1][2];
      for (int d = 0; d < 3; ++d) w[d] = A[1][d] - r01 * q0[d];
      const double r11 = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
      const double len1 = sqrt(A[1][0] * A[1][0] + A[1][1] * A[1][1] + A[1][2] * A[1][2]);
      if (r11 > LS_FLAT * len1) {   // r11 / |a1| is the sine of the corner angle
        v = 0.5 * r00 * r11;
        for (int d = 0; d < 3; ++d) {
          q1[d] = w[d] / r11;
          C[d][0] = q0[d] / r00 - q1[d] * r01 / (r00 * r11);
          C[d][1] = q1[d] / r11;
        }
      }
    }
  }
  if (!(v > 0.0)) v = 0.0;
  vol[e] = v;
  for (int d = 0; d < DX; ++d) {
    double s0 = 0.0;
    for (int s = 0; s < S; ++s) {
      s0 += C[d][s];
      cv[(e * K + s + 1) * DX + d] = (float)(C[d][s] * v);
    }
    cv[(e * K) * DX + d] = (float)(-s0 * v);
  }
}
// inv[n] = 1 / clamp(sum of the measures of the elements that contain n, 1e-12), in the order of the inverted index
__global__ void __launch_bounds__(256) k_ls_node_geom(const int64_t* __restrict__ nptr, const int32_t* __restrict__ nent, int K,
                                                      const double* __restrict__ vol, long N, float* __restrict__ inv) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  for (int64_t k = nptr[n]; k < nptr[n + 1]; ++k) s += vol[nent[k] / K];
  inv[n] = (float)(1.0 / fmax(s, 1e-12));
}

extern "C" int mgn_loss_fd_geometry(const int64_t* rowptr, const int32_t* col, const uint8_t* self_loop, const float* pos, int DX,
                                    int64_t N, float* coef, float* inv, void* stream) {
  if (rowptr == nullptr || pos == nullptr || inv == nullptr || N < 0 || DX < 1 || DX > LD)
    return fail(1, "mgn_loss_fd_geometry: bad arguments (positions of 1..3 columns)");
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_fd_geom, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, self_loop, pos, DX,
                     (long)N, coef, inv);
  return check_launch("mgn_loss_fd_geometry");
}
extern "C" int mgn_loss_ls_geometry(const int32_t* elems, int64_t M, int K, const float* pos, int DX, int64_t N, const int64_t* nptr,
                                    const int32_t* nent, float* cv, double* vol, float* inv, void* stream) {
  if (elems == nullptr || pos == nullptr || nptr == nullptr || nent == nullptr || cv == nullptr || vol == nullptr || inv == nullptr ||
      M < 0 || N < 0)
    return fail(1, "mgn_loss_ls_geometry: bad arguments");
  if (!((K == 3 && (DX == 2 || DX == 3)) || (K == 4 && DX == 3)))
    return fail(1, "mgn_loss_ls_geometry: elements are triangles in 2-D / 3-D or tetrahedra in 3-D");
  if (M * K >= ((int64_t)1 << 31)) return fail(1, "mgn_loss_ls_geometry: element corner count needs 32-bit entries");
  hipStream_t s = (hipStream_t)stream;
  if (M > 0) hipLaunchKernelGGL(k_ls_elem_geom, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, elems, (long)M, K, pos, DX, cv, vol);
  if (N > 0) hipLaunchKernelGGL(k_ls_node_geom, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, nptr, nent, K, (const double*)vol, (long)N, inv);
  return check_launch("mgn_loss_ls_geometry");
}

// ===================================================================== per step
__device__ __forceinline__ float smooth_l1(float d) {
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}
__device__ __forceinline__ float smooth_l1_grad(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }
__device__ __forceinline__ float sign0(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// least squares, element pass: ge[e, f, :] = sum_k U[elem[e, k], f] * cv[e, k, :]  (= grad_e * vol_e) for both fields, summed as
// sum_{k >= 1} (U[k] - U[0]) * cv[e, k, :] (cv[e, 0] is minus the sum of the others): the differences of neighbouring values are
// exact in fp32, the products of the values themselves would cancel
__global__ void __launch_bounds__(256) k_ls_elem_fwd(mgn_loss_args a) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.M) return;
  const int F = a.F, DX = a.DX, K = a.K;
  float go[LF][LD], gt[LF][LD], uo0[LF], ut0[LF];
  const long m0 = a.elems[e * K];
#pragma unroll
  for (int f = 0; f < LF; ++f) {
    uo0[f] = f < F ? a.u_out[m0 * F + f] : 0.f;
    ut0[f] = f < F ? a.u_tgt[m0 * F + f] : 0.f;
#pragma unroll
    for (int d = 0; d < LD; ++d) go[f][d] = gt[f][d] = 0.f;
  }
  for (int k = 1; k < K; ++k) {
    const long m = a.elems[e * K + k];
    float c[LD];
#pragma unroll
    for (int d = 0; d < LD; ++d) c[d] = d < DX ? a.cv[(e * K + k) * DX + d] : 0.f;
#pragma unroll
    for (int f = 0; f < LF; ++f)
      if (f < F) {
        const float uo = a.u_out[m * F + f] - uo0[f], ut = a.u_tgt[m * F + f] - ut0[f];
#pragma unroll
        for (int d = 0; d < LD; ++d) go[f][d] = fmaf(uo, c[d], go[f][d]), gt[f][d] = fmaf(ut, c[d], gt[f][d]);
      }
  }
#pragma unroll
  for (int f = 0; f < LF; ++f)
#pragma unroll
    for (int d = 0; d < LD; ++d)
      if (f < F && d < DX) a.ge_out[(e * F + f) * DX + d] = go[f][d], a.ge_tgt[(e * F + f) * DX + d] = gt[f][d];
}

// node pass: LG lanes share a node.  The lanes stride over the node's index entries -- consecutive lanes read consecutive
// entries, consecutive groups consecutive rows, so the entry stream is read in whole cache lines -- and their partial sums meet in
// a fixed butterfly (xor 1, 2, 4: every lane ends with the same bits).  Lane 0 of the group then evaluates the terms.
// part[t * LOSS_PART + block] = this block's sum of term t (unweighted, un-normalised); row nterms = selected-row count.
#define LG 8
#define NODES_PER_BLOCK (256 / LG)
__device__ __forceinline__ float grp_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}
template <int METHOD>
__global__ void __launch_bounds__(256) k_loss_node_fwd(mgn_loss_args a) {
  __shared__ float red[256];
  const int F = a.F, DX = a.DX, O = a.O, T = a.nterms;
  const float t0 = a.types[0], t1 = a.types[1], t2 = a.types[2], t3 = a.types[3];
  const bool physics = a.u_out != nullptr;
  const int lane = threadIdx.x & (LG - 1);
  float acc[MGN_LOSS_MAX_TERMS + 1];
#pragma unroll
  for (int t = 0; t <= MGN_LOSS_MAX_TERMS; ++t) acc[t] = 0.f;
  // (the loop bound is uniform over the block: every lane takes part in the shuffles)
  for (long base = (long)blockIdx.x * NODES_PER_BLOCK; base < a.N; base += (long)gridDim.x * NODES_PER_BLOCK) {
    const long n = base + threadIdx.x / LG;
    const bool valid = n < a.N;
    float Go[LF][LD], Gt[LF][LD], uo[LF], ut[LF], dG[LF][LD], dU[LF];
#pragma unroll
    for (int f = 0; f < LF; ++f) {
      uo[f] = ut[f] = dU[f] = 0.f;
#pragma unroll
      for (int d = 0; d < LD; ++d) Go[f][d] = Gt[f][d] = dG[f][d] = 0.f;
    }
    float invn = 0.f;
    if (physics) {
      if (valid) {
#pragma unroll
        for (int f = 0; f < LF; ++f)
          if (f < F) uo[f] = a.u_out[n * F + f], ut[f] = a.u_tgt[n * F + f];
        if (METHOD == 0) {
          for (int64_t k = a.rowptr[n] + lane; k < a.rowptr[n + 1]; k += LG) {
            const long m = a.col[k];
            float c[LD];
#pragma unroll
            for (int d = 0; d < LD; ++d) c[d] = d < DX ? a.coef[k * DX + d] : 0.f;
#pragma unroll
            for (int f = 0; f < LF; ++f)
              if (f < F) {
                const float du = a.u_out[m * F + f] - uo[f], dt = a.u_tgt[m * F + f] - ut[f];
#pragma unroll
                for (int d = 0; d < LD; ++d) Go[f][d] = fmaf(du, c[d], Go[f][d]), Gt[f][d] = fmaf(dt, c[d], Gt[f][d]);
              }
          }
        } else {
          for (int64_t k = a.nptr[n] + lane; k < a.nptr[n + 1]; k += LG) {
            const long e = a.nent[k] / a.K;
#pragma unroll
            for (int f = 0; f < LF; ++f)
#pragma unroll
              for (int d = 0; d < LD; ++d)
                if (f < F && d < DX) Go[f][d] += a.ge_out[(e * F + f) * DX + d], Gt[f][d] += a.ge_tgt[(e * F + f) * DX + d];
          }
        }
        invn = a.inv[n];
      }
#pragma unroll
      for (int f = 0; f < LF; ++f)
#pragma unroll
        for (int d = 0; d < LD; ++d)
          if (f < F && d < DX) Go[f][d] = grp_sum(Go[f][d]) * invn, Gt[f][d] = grp_sum(Gt[f][d]) * invn;
    }
    if (valid && lane == 0) {   // one lane per node from here: the terms, and what the backward needs
    const float ty = a.type[n * a.ldty];
    // a row listed in exclude leaves every mean; its field values were still gathered by its neighbours above
    const bool sel = (ty == t0 || ty == t1 || ty == t2 || ty == t3) && !(a.exclude != nullptr && a.exclude[n] != 0);
    if (physics && a.g_out != nullptr) {
#pragma unroll
      for (int f = 0; f < LF; ++f)
#pragma unroll
        for (int d = 0; d < LD; ++d)
          if (f < F && d < DX) a.g_out[(n * F + f) * DX + d] = Go[f][d];
    }
    bool bset = false;
    if (sel) acc[MGN_LOSS_MAX_TERMS] += 1.f;
#pragma unroll
    for (int t = 0; t < MGN_LOSS_MAX_TERMS; ++t) {
      if (t >= T) break;
      const int kind = a.term_type[t];
      const float w = a.term_weight[t];
      float v = 0.f;
      if (kind == MGN_LOSS_L2 || kind == MGN_LOSS_L1SMOOTH) {
        const float s = w / (float)O;
        for (int o = 0; o < O; ++o) {
          const float d = a.net_out[n * a.ld_out + o] - a.target[n * a.ld_tgt + o];
          float g;
          if (kind == MGN_LOSS_L2) v = fmaf(d, d, v), g = 2.f * d;
          else v += smooth_l1(d), g = smooth_l1_grad(d);
          const float prev = bset ? a.b_out[n * O + o] : 0.f;
          a.b_out[n * O + o] = sel ? prev + s * g : 0.f;
        }
        bset = true;
      } else if (kind == MGN_LOSS_COSINE) {   // 1 - <a,b> / sqrt((|a|^2 + 1e-12)(|b|^2 + 1e-12))
        float ab = 0.f, aa = 1e-12f, bb = 1e-12f;
        for (int o = 0; o < O; ++o) {
          const float x = a.net_out[n * a.ld_out + o], y = a.target[n * a.ld_tgt + o];
          ab = fmaf(x, y, ab), aa = fmaf(x, x, aa), bb = fmaf(y, y, bb);
        }
        const float den = sqrtf(aa * bb), cs = ab / den;
        v = 1.f - cs;
        for (int o = 0; o < O; ++o) {
          const float x = a.net_out[n * a.ld_out + o], y = a.target[n * a.ld_tgt + o];
          const float g = -(y / den - cs * x / aa);
          const float prev = bset ? a.b_out[n * O + o] : 0.f;
          a.b_out[n * O + o] = sel ? prev + w * g : 0.f;
        }
        bset = true;
      } else if (kind == MGN_LOSS_GRADIENT) {
        const float s = 2.f * w / (float)(F * DX);
#pragma unroll
        for (int f = 0; f < LF; ++f)
#pragma unroll
          for (int d = 0; d < LD; ++d)
            if (f < F && d < DX) {
              const float e = Go[f][d] - Gt[f][d];
              v = fmaf(e, e, v);
              dG[f][d] = fmaf(s, e, dG[f][d]);
            }
      } else if (kind == MGN_LOSS_CONVECTION) {   // c[f] = U[f] * sum_d G[f, d]
        const float s = 2.f * w / (float)F;
#pragma unroll
        for (int f = 0; f < LF; ++f)
          if (f < F) {
            float so = 0.f, st = 0.f;
#pragma unroll
            for (int d = 0; d < LD; ++d)
              if (d < DX) so += Go[f][d], st += Gt[f][d];
            const float e = uo[f] * so - ut[f] * st;
            v = fmaf(e, e, v);
            dU[f] = fmaf(s * e, so, dU[f]);
#pragma unroll
            for (int d = 0; d < LD; ++d)
              if (d < DX) dG[f][d] = fmaf(s * e, uo[f], dG[f][d]);
          }
      } else {   // the three divergence losses: div = sum_k G[k, k], k < min(F, DX)
        float div = 0.f;
#pragma unroll
        for (int k = 0; k < LD; ++k)
          if (k < F && k < DX) div += Go[k][k];
        float g;
        if (kind == MGN_LOSS_DIV_L2) v = div * div, g = 2.f * div;
        else if (kind == MGN_LOSS_DIV_L1) v = fabsf(div), g = sign0(div);
        else v = smooth_l1(div), g = smooth_l1_grad(div);
#pragma unroll
        for (int k = 0; k < LD; ++k)
          if (k < F && k < DX) dG[k][k] = fmaf(w, g, dG[k][k]);
      }
      if (sel) acc[t] += v;
    }
    if (physics) {   // what the backward gathers: inv[n] * dL/dG[n] (so the transposed pass reads no neighbour's inv) and the direct dL/dU[n]
#pragma unroll
      for (int f = 0; f < LF; ++f)
        if (f < F) {
          a.bu_out[n * F + f] = sel ? dU[f] : 0.f;
#pragma unroll
          for (int d = 0; d < LD; ++d)
            if (d < DX) a.a_out[(n * F + f) * DX + d] = sel ? invn * dG[f][d] : 0.f;
        }
    }
    }
  }
  // fixed-order block reduction of every row of the partial table
#pragma unroll
  for (int t = 0; t <= MGN_LOSS_MAX_TERMS; ++t) {
    if (t < T || t == MGN_LOSS_MAX_TERMS) {
      red[threadIdx.x] = acc[t];
      __syncthreads();
      for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
      }
      if (threadIdx.x == 0) a.part[(t == MGN_LOSS_MAX_TERMS ? T : t) * LOSS_PART + blockIdx.x] = red[0];
      __syncthreads();
    }
  }
}

// terms[t] = weight_t * sum_t / (count * elements per row of term t); total = their sum; invcount = 1 / count
__global__ void __launch_bounds__(256) k_loss_final(mgn_loss_args a, int nblk) {
  __shared__ double red[256];
  __shared__ double sums[MGN_LOSS_MAX_TERMS + 1];
  const int T = a.nterms;
  for (int t = 0; t <= T; ++t) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += (double)a.part[t * LOSS_PART + b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[t] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double cnt = sums[T];   // 0 selected rows: 0 / 0 = nan, as torch's mean of an empty selection
    double tot = 0.0;
    for (int t = 0; t < T; ++t) {
      const int kind = a.term_type[t];
      const double per = (kind == MGN_LOSS_L2 || kind == MGN_LOSS_L1SMOOTH) ? (double)a.O
                         : kind == MGN_LOSS_GRADIENT ? (double)(a.F * a.DX)
                         : kind == MGN_LOSS_CONVECTION ? (double)a.F : 1.0;
      const float v = (float)((double)a.term_weight[t] * sums[t] / (cnt * per));
      a.terms[t] = v;
      tot += (double)v;
    }
    *a.total = (float)tot;
    *a.invcount = (float)(1.0 / cnt);
  }
}

// least squares, backward element pass: dge[e, f, :] = sum_k a_out[elem[e, k], f, :]   (a_out carries 1 / sum vol of its node)
__global__ void __launch_bounds__(256) k_ls_elem_bwd(mgn_loss_args a, float* __restrict__ dge) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.M) return;
  const int FD = a.F * a.DX;
  float s[LF * LD];
#pragma unroll
  for (int i = 0; i < LF * LD; ++i) s[i] = 0.f;
  for (int k = 0; k < a.K; ++k) {
    const long m = a.elems[e * a.K + k];
#pragma unroll
    for (int i = 0; i < LF * LD; ++i)
      if (i < FD) s[i] += a.a_out[m * FD + i];
  }
#pragma unroll
  for (int i = 0; i < LF * LD; ++i)
    if (i < FD) dge[e * FD + i] = s[i];
}

// d_net[n, :] = g / count * b_out[n, :];   d_u[n, f] = g / count * (bu_out[n, f] + (transposed gradient operator applied to a_out)[n, f])
// LG lanes per node, as in the forward pass.
template <int METHOD>
__global__ void __launch_bounds__(256) k_loss_node_bwd(mgn_loss_args a, const float* __restrict__ g, float* __restrict__ d_net,
                                                       float* __restrict__ d_u, const float* __restrict__ dge) {
  const long n = (long)blockIdx.x * NODES_PER_BLOCK + threadIdx.x / LG;
  const int lane = threadIdx.x & (LG - 1);
  const bool valid = n < a.N;
  const float scale = (*g) * (*a.invcount);
  const int F = a.F, DX = a.DX, O = a.O;
  if (valid && d_net != nullptr)
    for (int o = lane; o < O; o += LG) d_net[n * O + o] = scale * a.b_out[n * O + o];
  if (d_u == nullptr) return;   // (uniform)
  float s[LF];
#pragma unroll
  for (int f = 0; f < LF; ++f) s[f] = 0.f;
  if (valid) {
    if (METHOD == 0) {   // G[n] = inv[n] sum_m (U[m] - U[n]) (x) c_nm and c_mn = -c_nm:  dU[n, f] = -sum_m (A[m, f, :] + A[n, f, :]) . c_nm
      float an[LF][LD];
#pragma unroll
      for (int f = 0; f < LF; ++f)
#pragma unroll
        for (int d = 0; d < LD; ++d) an[f][d] = (f < F && d < DX) ? a.a_out[(n * F + f) * DX + d] : 0.f;
      for (int64_t k = a.rowptr[n] + lane; k < a.rowptr[n + 1]; k += LG) {
        const long m = a.col[k];
        float c[LD];
#pragma unroll
        for (int d = 0; d < LD; ++d) c[d] = d < DX ? a.coef[k * DX + d] : 0.f;
#pragma unroll
        for (int f = 0; f < LF; ++f)
#pragma unroll
          for (int d = 0; d < LD; ++d)
            if (f < F && d < DX) s[f] = fmaf(-(a.a_out[(m * F + f) * DX + d] + an[f][d]), c[d], s[f]);
      }
    } else {
      for (int64_t k = a.nptr[n] + lane; k < a.nptr[n + 1]; k += LG) {
        const long ent = a.nent[k], e = ent / a.K;
#pragma unroll
        for (int f = 0; f < LF; ++f)
#pragma unroll
          for (int d = 0; d < LD; ++d)
            if (f < F && d < DX) s[f] = fmaf(dge[(e * F + f) * DX + d], a.cv[ent * DX + d], s[f]);
      }
    }
  }
#pragma unroll
  for (int f = 0; f < LF; ++f)
    if (f < F) s[f] = grp_sum(s[f]);
  if (valid && lane == 0) {
#pragma unroll
    for (int f = 0; f < LF; ++f)
      if (f < F) d_u[n * F + f] = scale * (a.bu_out[n * F + f] + s[f]);
  }
}

static int loss_validate(const mgn_loss_args* a, const char** why) {
  *why = nullptr;
  if (a == nullptr) { *why = "null arguments"; return 1; }
  if (a->N < 0 || a->O < 1 || a->net_out == nullptr || a->target == nullptr || a->type == nullptr || a->ntypes < 1 || a->ntypes > 4) {
    *why = "needs output, target and node type rows and 1..4 node types"; return 1;
  }
  if (a->nterms < 1 || a->nterms > MGN_LOSS_MAX_TERMS) { *why = "1..8 loss terms"; return 1; }
  if (a->part == nullptr || a->terms == nullptr || a->total == nullptr || a->invcount == nullptr || a->b_out == nullptr) {
    *why = "missing output or workspace pointer"; return 1;
  }
  bool physics = false;
  for (int t = 0; t < a->nterms; ++t) {
    if (a->term_type[t] < MGN_LOSS_L2 || a->term_type[t] > MGN_LOSS_DIV_L1SMOOTH) { *why = "unknown loss term"; return 1; }
    physics = physics || a->term_type[t] >= MGN_LOSS_GRADIENT;
  }
  if (physics && a->u_out == nullptr) { *why = "a physics term needs the physical fields"; return 1; }
  if (a->u_out != nullptr) {
    if (a->u_tgt == nullptr || a->a_out == nullptr || a->bu_out == nullptr || a->inv == nullptr) { *why = "physical fields without their buffers"; return 1; }
    if (a->F < 1 || a->F > LF || a->DX < 1 || a->DX > LD) { *why = "fields of 1..4 columns, positions of 1..3"; return 1; }
    if (a->method == MGN_LOSS_FINITE_DIFF) {
      if (a->rowptr == nullptr || (a->col == nullptr && a->N > 0) ) { *why = "finite_diff needs the neighbour CSR"; return 1; }
    } else if (a->method == MGN_LOSS_LEAST_SQUARES) {
      if (a->elems == nullptr || a->cv == nullptr || a->nptr == nullptr || a->nent == nullptr || a->ge_out == nullptr || a->ge_tgt == nullptr ||
          a->M < 0 || (a->K != 3 && a->K != 4)) { *why = "least_squares needs the element tables"; return 1; }
    } else { *why = "unknown gradient method"; return 1; }
  }
  return 0;
}

extern "C" size_t mgn_loss_workspace_bytes(void) { return (size_t)(MGN_LOSS_MAX_TERMS + 1) * LOSS_PART * sizeof(float); }

extern "C" int mgn_loss_fwd(const mgn_loss_args* args, void* stream) {
  const char* why;
  if (loss_validate(args, &why)) {
    snprintf(g_err, sizeof(g_err), "mgn_loss_fwd: %s", why);
    return 1;
  }
  mgn_loss_args a = *args;
  for (int k = a.ntypes; k < 4; ++k) a.types[k] = a.types[0];
  hipStream_t s = (hipStream_t)stream;
  int nblk = (int)((a.N + NODES_PER_BLOCK - 1) / NODES_PER_BLOCK);
  if (nblk > LOSS_PART) nblk = LOSS_PART;
  if (nblk < 1) nblk = 1;
  const bool ls = a.u_out != nullptr && a.method == MGN_LOSS_LEAST_SQUARES;
  if (ls && a.M > 0) hipLaunchKernelGGL(k_ls_elem_fwd, dim3((unsigned)((a.M + 255) / 256)), dim3(256), 0, s, a);
  if (ls) hipLaunchKernelGGL(k_loss_node_fwd<1>, dim3(nblk), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_loss_node_fwd<0>, dim3(nblk), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(256), 0, s, a, nblk);
  return check_launch("mgn_loss_fwd");
}

extern "C" int mgn_loss_bwd(const mgn_loss_args* args, const float* g, float* d_net, float* d_u, float* dge, void* stream) {
  const char* why;
  if (loss_validate(args, &why)) {
    snprintf(g_err, sizeof(g_err), "mgn_loss_bwd: %s", why);
    return 1;
  }
  if (g == nullptr || (d_net == nullptr && d_u == nullptr)) return fail(1, "mgn_loss_bwd: needs the incoming gradient and an output");
  mgn_loss_args a = *args;
  if (d_u != nullptr && a.u_out == nullptr) return fail(1, "mgn_loss_bwd: no physical fields in this loss");
  const bool ls = d_u != nullptr && a.method == MGN_LOSS_LEAST_SQUARES;
  if (ls && dge == nullptr) return fail(1, "mgn_loss_bwd: least_squares needs the [M, F, DX] scratch");
  if (a.N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)((a.N + NODES_PER_BLOCK - 1) / NODES_PER_BLOCK);
  if (ls && a.M > 0) hipLaunchKernelGGL(k_ls_elem_bwd, dim3((unsigned)((a.M + 255) / 256)), dim3(256), 0, s, a, dge);
  if (ls) hipLaunchKernelGGL(k_loss_node_bwd<1>, dim3(nb), dim3(256), 0, s, a, g, d_net, d_u, (const float*)dge);
  else hipLaunchKernelGGL(k_loss_node_bwd<0>, dim3(nb), dim3(256), 0, s, a, g, d_net, d_u, (const float*)dge);
  return check_launch("mgn_loss_bwd");
}
