// MI355X (gfx950) exact k-nearest-neighbour search and inverse-distance interpolation: what the reference's multigrid pooling
// (graphphysics/models/hierarchical_pooling.py: PyG KNNGraph and knn_interpolate, both on torch_cluster.knn) and its
// compute_min_distance_to_type (dataset/preprocessing.py:241-274) need.  Ninth translation unit of libmgn_hip.so.  The result
// contract (include/mgn_hip.h, mgn_knn_search) pins every bit: tests/knn_reference.py restates it in numpy.
//
//   search  brute force, one lane = one query, all lanes of a workgroup in ONE segment (graph of the batch).  Workgroup b finds
//           its (segment, first query) by walking ptr_y -- nseg uniform loads, no table, no workspace; the grid
//           ceil(ny / 256) + nseg is an upper bound the host knows without a synchronisation, surplus workgroups leave at once.
//           The segment's reference points stream through LDS in structure-of-arrays tiles of KNN_TILE points; every lane reads
//           the same four points with one ds_read_b128 per coordinate (same address in all lanes: a broadcast, no conflicts).
//           Each lane keeps its best CAP (template: 1, 4, 8, 16, 32) as a sorted list in registers; a candidate enters through
//           an unrolled compare-and-shift chain with compile-time slot numbers only (no scratch), and a wave skips the chain
//           when none of its lanes beats its current worst (__any).  References arrive in ascending index order and a
//           candidate enters only when STRICTLY nearer than a slot, so equal distances keep the lower index in front: the order
//           is (d2, index) whatever the tile size or the grid.
//   interp  k_knn_weights: one lane per query, a_j = w_j / sum w_j, w_j = 1 / max(d2_j, 1e-16) (PyG 2.6.1 knn_interpolate);
//           k_knn_interp_fwd: one lane per output element, fp32 fma in slot order; k_knn_interp_bwd: one lane per element of
//           dx, a segment sum over the CSR of the assignment keyed by reference node (mgn_csr_build: slots in ascending
//           order) -- no atomics, bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "mgn_hip.h"

#include "mgn_host.inc"  // g_err, fail, check_launch
extern "C" const char* mgn_knn_last_error(void) { return g_err; }

#define KNN_THREADS 256
#define KNN_TILE 1024  // reference points per LDS tile: 4 KiB per coordinate
#define KNN_MAXK 32
#define KNN_NMAX 2147483647LL

extern "C" int mgn_knn_max_k(void) { return KNN_MAXK; }
extern "C" int mgn_knn_tile_points(void) { return KNN_TILE; }

// ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded once.  __fmul_rn / __fadd_rn of this toolchain are the plain
// operators, so what keeps the products out of an FMA is the pragma: no contraction inside this function.
template <int DIM>
__device__ __forceinline__ float knn_d2(const float (&q)[3], float rx, float ry, float rz) {
#pragma clang fp contract(off)
  const float dx = q[0] - rx, dy = q[1] - ry;
  float d = (dx * dx) + (dy * dy);
  if (DIM == 3) {
    const float dz = q[2] - rz;
    d = d + (dz * dz);
  }
  return d;
}

// (d, gi) enters the sorted list behind every entry with distance <= d.  Top-down compare-and-shift, slot numbers are
// compile-time constants: the lists stay in registers.
template <int CAP>
__device__ __forceinline__ void knn_insert(float (&bd)[CAP], int (&bi)[CAP], float d, int gi) {
#pragma unroll
  for (int s = CAP - 1; s >= 1; --s) {
    const bool shift = d < bd[s - 1], here = d < bd[s];
    bi[s] = shift ? bi[s - 1] : (here ? gi : bi[s]);
    bd[s] = shift ? bd[s - 1] : (here ? d : bd[s]);
  }
  if (d < bd[0]) {
    bd[0] = d;
    bi[0] = gi;
  }
}

__device__ __forceinline__ long knn_clamp(int64_t v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : (long)v); }

template <int CAP, int DIM>
__global__ void __launch_bounds__(KNN_THREADS) k_knn_search(const float* __restrict__ x, const float* __restrict__ y,
                                                            const int64_t* __restrict__ ptr_x, const int64_t* __restrict__ ptr_y, int nseg,
                                                            long nx, long ny, int k, int exclude_self, int64_t* __restrict__ idx,
                                                            float* __restrict__ d2) {
  __shared__ __attribute__((aligned(16))) float s_c[DIM][KNN_TILE];
  // the segment of this workgroup: segment s owns ceil(ny_s / KNN_THREADS) consecutive workgroups.  Offsets are clamped to the
  // arrays and made monotone, so a damaged ptr cannot lead outside them.
  long first = 0, q0 = 0, qend = 0, lo = knn_clamp(ptr_y[0], 0, ny);
  int seg = -1;
  for (int s = 0; s < nseg; ++s) {
    const long hi = knn_clamp(ptr_y[s + 1], lo, ny);
    const long nb = (hi - lo + KNN_THREADS - 1) / KNN_THREADS;
    if ((long)blockIdx.x < first + nb) {
      seg = s, q0 = lo + ((long)blockIdx.x - first) * KNN_THREADS, qend = hi;
      break;
    }
    first += nb, lo = hi;
  }
  if (seg < 0) return;  // surplus workgroup of the upper-bound grid (uniform: before any barrier)
  const long x0 = knn_clamp(ptr_x[seg], 0, nx), x1 = knn_clamp(ptr_x[seg + 1], x0, nx);
  const long q = q0 + threadIdx.x;
  const bool active = q < qend;
  float qc[3] = {0.f, 0.f, 0.f};
  if (active) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) qc[d] = y[q * DIM + d];
  }
  float bd[CAP];
  int bi[CAP];
#pragma unroll
  for (int s = 0; s < CAP; ++s) bd[s] = active ? INFINITY : -INFINITY, bi[s] = -1;  // an idle lane never has a candidate
  const int self = (exclude_self && active) ? (int)q : -1;

  for (long t = x0; t < x1; t += KNN_TILE) {
    const int cnt = (int)((x1 - t) < KNN_TILE ? (x1 - t) : KNN_TILE);
    const int cnt4 = (cnt + 3) & ~3;
    __syncthreads();  // the previous tile has been read by every wave
    for (int p = threadIdx.x; p < cnt4; p += KNN_THREADS) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) s_c[d][p] = p < cnt ? x[(t + p) * DIM + d] : NAN;  // padding: NaN never compares below
    }
    __syncthreads();
    for (int j = 0; j < cnt4; j += 4) {
      const float4 rx = *reinterpret_cast<const float4*>(&s_c[0][j]);
      const float4 ry = *reinterpret_cast<const float4*>(&s_c[1][j]);
      float4 rz = make_float4(0.f, 0.f, 0.f, 0.f);
      if (DIM == 3) rz = *reinterpret_cast<const float4*>(&s_c[DIM - 1][j]);
      const float e0 = knn_d2<DIM>(qc, rx.x, ry.x, rz.x), e1 = knn_d2<DIM>(qc, rx.y, ry.y, rz.y);
      const float e2 = knn_d2<DIM>(qc, rx.z, ry.z, rz.z), e3 = knn_d2<DIM>(qc, rx.w, ry.w, rz.w);
      const float worst = bd[CAP - 1];
      if (__any((e0 < worst) | (e1 < worst) | (e2 < worst) | (e3 < worst))) {
        const int g = (int)(t + j);
        if (e0 < bd[CAP - 1] && g != self) knn_insert<CAP>(bd, bi, e0, g);
        if (e1 < bd[CAP - 1] && g + 1 != self) knn_insert<CAP>(bd, bi, e1, g + 1);
        if (e2 < bd[CAP - 1] && g + 2 != self) knn_insert<CAP>(bd, bi, e2, g + 2);
        if (e3 < bd[CAP - 1] && g + 3 != self) knn_insert<CAP>(bd, bi, e3, g + 3);
      }
    }
  }
  if (active) {
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
      if (s < k) {
        idx[q * k + s] = (int64_t)bi[s];
        d2[q * k + s] = bd[s];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- interpolation
__global__ void __launch_bounds__(256) k_knn_weights(const int64_t* __restrict__ idx, const float* __restrict__ d2, long ny, long nx, int k,
                                                     float* __restrict__ a) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < ny; r += (long)gridDim.x * blockDim.x) {
    float sum = 0.f;
    for (int j = 0; j < k; ++j) {
      const int64_t c = idx[r * k + j];
      if (c >= 0 && c < nx) sum += 1.0f / fmaxf(d2[r * k + j], 1e-16f);
    }
    for (int j = 0; j < k; ++j) {
      const int64_t c = idx[r * k + j];
      a[r * k + j] = (c >= 0 && c < nx) ? (1.0f / fmaxf(d2[r * k + j], 1e-16f)) / sum : 0.f;
    }
  }
}

__global__ void __launch_bounds__(256) k_knn_interp_fwd(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                                        const float* __restrict__ a, long ny, long nx, int k, int F, float* __restrict__ out) {
  const long total = ny * F;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long r = e / F;
    const int f = (int)(e - r * F);
    float acc = 0.f;
    for (int j = 0; j < k; ++j) {
      const int64_t c = idx[r * k + j];
      if (c >= 0 && c < nx) acc = __fmaf_rn(a[r * k + j], x[c * F + f], acc);
    }
    out[e] = acc;
  }
}

__global__ void __launch_bounds__(256) k_knn_interp_bwd(const float* __restrict__ dy, const float* __restrict__ a,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm, long nx, long ny,
                                                        int k, int F, float* __restrict__ dx) {
  const long total = nx * F, slots = ny * k;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long c = e / F;
    const int f = (int)(e - c * F);
    long b0 = rowptr[c], b1 = rowptr[c + 1];
    b0 = b0 < 0 ? 0 : b0, b1 = b1 > slots ? slots : b1;
    float acc = 0.f;
    for (long i = b0; i < b1; ++i) {
      const long s = perm[i];
      if (s >= 0 && s < slots) acc = __fmaf_rn(a[s], dy[(s / k) * F + f], acc);
    }
    dx[e] = acc;
  }
}

// ---------------------------------------------------------------------------------------- host side
static unsigned knn_grid(long items) {
  const long nb = (items + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : (nb > 65536 ? 65536 : nb));  // grid-stride beyond
}

template <int DIM>
static void knn_launch(int k, dim3 grid, hipStream_t s, const float* x, const float* y, const int64_t* ptr_x, const int64_t* ptr_y, int nseg,
                       long nx, long ny, int excl, int64_t* idx, float* d2) {
#define KNN_GO(CAP) \
  hipLaunchKernelGGL((k_knn_search<CAP, DIM>), grid, dim3(KNN_THREADS), 0, s, x, y, ptr_x, ptr_y, nseg, nx, ny, k, excl, idx, d2)
  if (k == 1) KNN_GO(1);
  else if (k <= 4) KNN_GO(4);
  else if (k <= 8) KNN_GO(8);
  else if (k <= 16) KNN_GO(16);
  else KNN_GO(32);
#undef KNN_GO
}

extern "C" int mgn_knn_search(const float* x, int64_t nx, const float* y, int64_t ny, int dim, int k, const int64_t* ptr_x,
                              const int64_t* ptr_y, int64_t nseg, int exclude_self, int64_t* idx, float* d2, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dim != 2 && dim != 3) return fail(1, "mgn_knn_search: dim must be 2 or 3");
  if (k < 1) return fail(1, "mgn_knn_search: k must be >= 1");
  if (k > KNN_MAXK) return fail(1, "mgn_knn_search: k must not exceed mgn_knn_max_k() = 32");
  if (nseg < 1 || nseg > KNN_NMAX) return fail(1, "mgn_knn_search: nseg must be in [1, 2^31 - 1]");
  if (nx < 0 || nx > KNN_NMAX || ny < 0 || ny > KNN_NMAX) return fail(1, "mgn_knn_search: nx and ny must be in [0, 2^31 - 1]");
  if (ny * k > KNN_NMAX) return fail(1, "mgn_knn_search: ny * k must be below 2^31");
  if (!ptr_x || !ptr_y) return fail(1, "mgn_knn_search: ptr_x / ptr_y must not be null");
  if (nx > 0 && !x) return fail(1, "mgn_knn_search: x must not be null");
  if (ny > 0 && (!y || !idx || !d2)) return fail(1, "mgn_knn_search: y / idx / d2 must not be null");
  if (ny == 0) return 0;
  const long nb = (long)((ny + KNN_THREADS - 1) / KNN_THREADS + nseg);
  if (nb > KNN_NMAX) return fail(1, "mgn_knn_search: too many workgroups");
  const dim3 grid((unsigned)nb);
  if (dim == 2) knn_launch<2>(k, grid, s, x, y, ptr_x, ptr_y, (int)nseg, (long)nx, (long)ny, exclude_self ? 1 : 0, idx, d2);
  else knn_launch<3>(k, grid, s, x, y, ptr_x, ptr_y, (int)nseg, (long)nx, (long)ny, exclude_self ? 1 : 0, idx, d2);
  return check_launch("mgn_knn_search");
}

extern "C" int mgn_knn_interp_fwd(const float* x, int64_t nx, int F, const int64_t* idx, const float* d2, int64_t ny, int k, float* a,
                                  float* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (F < 1) return fail(1, "mgn_knn_interp_fwd: F must be >= 1");
  if (k < 1 || k > KNN_MAXK) return fail(1, "mgn_knn_interp_fwd: k must be in [1, mgn_knn_max_k()]");
  if (nx < 0 || nx > KNN_NMAX || ny < 0 || ny > KNN_NMAX || ny * k > KNN_NMAX) return fail(1, "mgn_knn_interp_fwd: nx, ny, ny * k must be in [0, 2^31 - 1]");
  if (nx > 0 && !x) return fail(1, "mgn_knn_interp_fwd: x must not be null");
  if (ny > 0 && (!idx || !d2 || !a || !out)) return fail(1, "mgn_knn_interp_fwd: idx / d2 / a / out must not be null");
  if (ny == 0) return 0;
  hipLaunchKernelGGL(k_knn_weights, dim3(knn_grid((long)ny)), dim3(256), 0, s, idx, d2, (long)ny, (long)nx, k, a);
  hipLaunchKernelGGL(k_knn_interp_fwd, dim3(knn_grid((long)ny * F)), dim3(256), 0, s, x, idx, (const float*)a, (long)ny, (long)nx, k, F, out);
  return check_launch("mgn_knn_interp_fwd");
}

extern "C" int mgn_knn_interp_bwd(const float* dy, const float* a, const int32_t* rowptr, const int32_t* perm, int64_t nx, int64_t ny, int k,
                                  int F, float* dx, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (F < 1) return fail(1, "mgn_knn_interp_bwd: F must be >= 1");
  if (k < 1 || k > KNN_MAXK) return fail(1, "mgn_knn_interp_bwd: k must be in [1, mgn_knn_max_k()]");
  if (nx < 0 || nx > KNN_NMAX || ny < 0 || ny > KNN_NMAX || ny * k > KNN_NMAX) return fail(1, "mgn_knn_interp_bwd: nx, ny, ny * k must be in [0, 2^31 - 1]");
  if (nx > 0 && (!rowptr || !dx)) return fail(1, "mgn_knn_interp_bwd: rowptr / dx must not be null");
  if (nx > 0 && ny > 0 && (!dy || !a || !perm)) return fail(1, "mgn_knn_interp_bwd: dy / a / perm must not be null");
  if (nx == 0) return 0;
  hipLaunchKernelGGL(k_knn_interp_bwd, dim3(knn_grid((long)nx * F)), dim3(256), 0, s, dy, a, rowptr, perm, (long)nx, (long)ny, k, F, dx);
  return check_launch("mgn_knn_interp_bwd");
}
