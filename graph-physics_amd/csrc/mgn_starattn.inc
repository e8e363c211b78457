// The spatial multi-token-prediction branch (training.use_spatial_mtp), included by mgn_attn.hip (the error channel comes from
// there); declared in include/mgn_hip_mtp.h.
//
// The reference (graphphysics/models/spatial_mtp_1hop.py) pads every star -- a centre node and its 1-hop neighbours -- to
// 1 + max_deg rows of a [B, L, d] tensor and masks the padding.  A padded key is masked and a padded query is never read, so the
// same mathematics runs on PACKED rows: star b owns rows [off[b], off[b+1]) of one [R, d] matrix.  The work is small (256 stars of
// about 7 rows at d = 128): what counts is the number of launches and their latency, not throughput.
//
//   k_star_offsets    one workgroup: degrees (capped), their running sum off[B+1], R, the pair count and the largest degree
//   k_star_cap        one workgroup per star: the max_neighbors smallest of c Philox keys (a rank count, c^2 compares)
//   k_star_pack       one workgroup per star, one wave per row: gather, RMSNorm, the index tables of the later steps
//   k_star_attn_fwd   one workgroup per star.  SA_TQ query rows at a time; keys and values stream through LDS in tiles of SA_T rows
//                     with a running maximum and sum per (query, head).  Scores: one thread per (query, head, key); outputs: one
//                     thread per (query, column).  fp32 VALU: a star's scores are a 7 x 7 matrix per head, far below an MFMA tile
//   k_star_attn_bwd   two workgroups per star: y = 0 forms dQ (query tiles outside, key tiles inside), y = 1 forms dK and dV (key
//                     tiles outside, query tiles inside).  Each output element has one owner thread: no atomics
//   k_star_loss       one workgroup: one thread per star walks its rows, fp64 sums, a fixed tree over the threads
//
// Fixed orders everywhere: the same bits on every run.
#include "mgn_hip_mtp.h"
#include "mgn_philox.inc"

#define SA_T 16       // key / value rows per LDS tile (mgn_star_attn_tile_rows)
#define SA_TQ 8       // query rows per pass
#define SA_MAXD 128   // widest row
#define SA_MAXH 16    // most heads
#define SA_ROW_LIMIT ((int64_t)(0x7fffffff / (3 * SA_MAXD)))

static_assert(SA_TQ * SA_MAXD == 4 * 256, "k_star_attn_fwd keeps 4 outputs per thread");
static_assert(SA_T * SA_MAXD == 8 * 256, "k_star_attn_bwd keeps 8 dK and 8 dV elements per thread");
static_assert(SA_TQ * SA_MAXH <= 256, "one thread per (query, head) of a pass");

// ------------------------------------------------------------------------------------------------ offsets
__global__ void __launch_bounds__(256) k_star_offsets(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ centers, int N, int B,
                                                      int cap, int32_t* __restrict__ off, int32_t* __restrict__ meta,
                                                      float* __restrict__ stats) {
  __shared__ long s_scan[256];
  __shared__ int s_max[256];
  __shared__ int s_bad[256];
  const int tid = threadIdx.x;
  long carry = 0;
  int mx = 0, bad = 0;
  if (tid == 0) off[0] = 0;
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + tid;
    long v = 0;
    if (b < B) {
      const int c = centers[b];
      int deg = 0;
      if (c >= 0 && c < N) {
        deg = rowptr[c + 1] - rowptr[c];
        if (deg < 0) deg = 0;
        if (cap > 0 && deg > cap) deg = cap;
      } else {
        bad = 1;
      }
      mx = deg > mx ? deg : mx;
      v = 1 + deg;
    }
    s_scan[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the chunk
      const long add = tid >= o ? s_scan[tid - o] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    const long incl = carry + s_scan[tid];
    if (b < B) off[b + 1] = incl > 0x7fffffffL ? 0x7fffffff : (int32_t)incl;
    carry += s_scan[255];
    __syncthreads();
  }
  s_max[tid] = mx, s_bad[tid] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      s_max[tid] = s_max[tid + o] > s_max[tid] ? s_max[tid + o] : s_max[tid];
      s_bad[tid] |= s_bad[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool big = carry > SA_ROW_LIMIT;
    meta[0] = big ? 0x7fffffff : (int32_t)carry;
    meta[1] = (s_bad[0] ? 1 : 0) | (big ? 2 : 0);
    stats[0] = (float)(carry - B);
    stats[1] = (float)s_max[0];
  }
}

extern "C" int mgn_star_offsets(const int32_t* rowptr, const int32_t* centers, int64_t N, int64_t B, int max_neighbors, int32_t* off,
                                int32_t* meta, float* stats, void* stream) {
  if (rowptr == nullptr || off == nullptr || meta == nullptr || stats == nullptr || (centers == nullptr && B > 0))
    return fail(1, "mgn_star_offsets: null pointer");
  if (N < 0 || N >= 0x7fffffff || B < 0 || B > SA_ROW_LIMIT) return fail(1, "mgn_star_offsets: node or centre count out of range");
  hipLaunchKernelGGL(k_star_offsets, dim3(1), dim3(256), 0, (hipStream_t)stream, rowptr, centers, (int)N, (int)B, max_neighbors, off, meta,
                     stats);
  return check_launch("mgn_star_offsets");
}

// ------------------------------------------------------------------------------------------------ cap
#define SA_CAP_KEYS 2048  // keys of a star kept in LDS; a longer row recomputes the rest

__device__ __forceinline__ uint64_t star_key(uint32_t k0, uint32_t k1, uint32_t j, uint32_t b, uint32_t step) {
  uint32_t r0, r1;
  philox4x32_10(k0, k1, j, b, step, 0x4d5450u, r0, r1);
  return ((uint64_t)r0 << 32) | r1;
}

__global__ void __launch_bounds__(256) k_star_cap(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ centers,
                                                  const int32_t* __restrict__ off, int N, int cap, uint32_t k0, uint32_t k1, uint32_t step,
                                                  int32_t* __restrict__ keep) {
  __shared__ uint64_t s_key[SA_CAP_KEYS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ctr = centers[b];
  if (ctr < 0 || ctr >= N) return;
  const int c = rowptr[ctr + 1] - rowptr[ctr];
  const int kept = off[b + 1] - off[b] - 1;
  int32_t* out = keep + (off[b] - b);
  if (c <= cap || kept != cap) {  // keeps all its neighbours, in order (a table that disagrees with the cap is left in order too)
    for (int j = tid; j < kept; j += 256) out[j] = j;
    return;
  }
  const int cached = c < SA_CAP_KEYS ? c : SA_CAP_KEYS;
  for (int j = tid; j < cached; j += 256) s_key[j] = star_key(k0, k1, (uint32_t)j, (uint32_t)b, step);
  __syncthreads();
  for (int j = tid; j < c; j += 256) {
    const uint64_t mine = j < cached ? s_key[j] : star_key(k0, k1, (uint32_t)j, (uint32_t)b, step);
    int rank = 0;
    for (int o = 0; o < c; ++o) {
      const uint64_t other = o < cached ? s_key[o] : star_key(k0, k1, (uint32_t)o, (uint32_t)b, step);
      rank += (other < mine || (other == mine && o < j)) ? 1 : 0;
    }
    if (rank < cap) out[rank] = j;
  }
}

extern "C" int mgn_star_cap(const int32_t* rowptr, const int32_t* centers, const int32_t* off, int64_t N, int64_t B, int max_neighbors,
                            uint64_t seed, uint32_t step, int32_t* keep, void* stream) {
  if (rowptr == nullptr || centers == nullptr || off == nullptr || keep == nullptr) return fail(1, "mgn_star_cap: null pointer");
  if (max_neighbors < 1) return fail(1, "mgn_star_cap: max_neighbors must be at least 1");
  if (N < 0 || N >= 0x7fffffff || B < 0 || B > SA_ROW_LIMIT) return fail(1, "mgn_star_cap: node or centre count out of range");
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_star_cap, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, rowptr, centers, off, (int)N, max_neighbors,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), step, keep);
  return check_launch("mgn_star_cap");
}

// ------------------------------------------------------------------------------------------------ pack
__global__ void __launch_bounds__(256) k_star_pack(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
                                                   const int32_t* __restrict__ centers, const int32_t* __restrict__ off,
                                                   const int32_t* __restrict__ keep, const float* __restrict__ H,
                                                   const float* __restrict__ Hn, const float* __restrict__ scale, int N, int B, int R, int d,
                                                   long key_offset, int32_t* __restrict__ row_node, int32_t* __restrict__ row_star,
                                                   int64_t* __restrict__ row_key, int32_t* __restrict__ nb_rows,
                                                   int32_t* __restrict__ nb_ptr, float* __restrict__ X0, float* __restrict__ X,
                                                   float* __restrict__ inv_out) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int s0 = off[b], s1 = off[b + 1];
  if (s0 < 0) s0 = 0;
  if (s1 > R) s1 = R;
  if (b == B - 1 && threadIdx.x == 0) nb_ptr[R] = R - B;
  const int ctr = centers[b];
  const bool ctr_ok = ctr >= 0 && ctr < N;
  const int base = ctr_ok ? rowptr[ctr] : 0;
  const int cnt = ctr_ok ? rowptr[ctr + 1] - base : 0;
  const float rd = sqrtf((float)d);
  for (int r = s0 + wv; r < s1; r += 4) {
    const int t = r - s0;
    int node = -1;
    if (t == 0) {
      node = ctr_ok ? ctr : -1;
    } else {
      const int p = keep != nullptr ? keep[r - b - 1] : t - 1;
      if (p >= 0 && p < cnt) node = nbr[base + p];
      if (node < 0 || node >= N) node = -1;
    }
    const float* src = (t == 0 ? H : Hn) + (size_t)(node < 0 ? 0 : node) * d;
    const int c0 = lane, c1 = lane + 64;
    const float x0 = (node >= 0 && c0 < d) ? src[c0] : 0.f;
    const float x1 = (node >= 0 && c1 < d) ? src[c1] : 0.f;
    float ss = fmaf(x0, x0, x1 * x1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float inv = 1.0f / (sqrtf(ss) / rd + 1e-8f);
    if (c0 < d) X0[(size_t)r * d + c0] = x0, X[(size_t)r * d + c0] = scale[c0] * (x0 * inv);
    if (c1 < d) X0[(size_t)r * d + c1] = x1, X[(size_t)r * d + c1] = scale[c1] * (x1 * inv);
    if (lane == 0) {
      row_node[r] = node;
      row_star[r] = b;
      row_key[r] = (long)(node < 0 ? 0 : node) + (t == 0 ? key_offset : 0);
      inv_out[r] = inv;
      nb_ptr[r] = r - b - (t == 0 ? 0 : 1);
      if (t > 0) nb_rows[r - b - 1] = r;
    }
  }
}

static int star_d_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }

extern "C" int mgn_star_pack(const int32_t* rowptr, const int32_t* nbr, const int32_t* centers, const int32_t* off, const int32_t* keep,
                             const float* H, const float* H_neigh, const float* scale, int64_t N, int64_t B, int64_t R, int d,
                             int64_t key_offset, int32_t* row_node, int32_t* row_star, int64_t* row_key, int32_t* nb_rows, int32_t* nb_ptr,
                             float* X0, float* X, float* inv, void* stream) {
  if (!star_d_ok(d)) return fail(1, "mgn_star_pack: d must be 16, 32, 64 or 128");
  if (N < 0 || N >= 0x7fffffff || B < 0 || R < B || R > SA_ROW_LIMIT || key_offset < 0)
    return fail(1, "mgn_star_pack: node, centre or row count out of range");
  if (R == 0 || B == 0) return 0;
  if (rowptr == nullptr || centers == nullptr || off == nullptr || H == nullptr || H_neigh == nullptr || scale == nullptr ||
      row_node == nullptr || row_star == nullptr || row_key == nullptr || nb_ptr == nullptr || X0 == nullptr || X == nullptr ||
      inv == nullptr || (R > B && (nbr == nullptr || nb_rows == nullptr)))
    return fail(1, "mgn_star_pack: null pointer");
  hipLaunchKernelGGL(k_star_pack, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, rowptr, nbr, centers, off, keep, H, H_neigh, scale,
                     (int)N, (int)B, (int)R, d, (long)key_offset, row_node, row_star, row_key, nb_rows, nb_ptr, X0, X, inv);
  return check_launch("mgn_star_pack");
}

// ------------------------------------------------------------------------------------------------ attention forward
// LDS index of the score of (query i, head h, key j) of the current tile pair
#define SA_S(i, h, j) ((((i) * SA_MAXH) + (h)) * SA_T + (j))

__global__ void __launch_bounds__(256) k_star_attn_fwd(const float* __restrict__ qkv, const int32_t* __restrict__ off, int R, int d,
                                                       int heads, float* __restrict__ y, float* __restrict__ lse) {
  __shared__ float sQ[SA_TQ][SA_MAXD];
  __shared__ float sK[SA_T][SA_MAXD + 1];  // (+1: a score thread walks a row, neighbouring threads neighbouring rows)
  __shared__ float sV[SA_T][SA_MAXD];
  __shared__ float sS[SA_TQ * SA_MAXH * SA_T];
  __shared__ float sM[SA_TQ * SA_MAXH], sL[SA_TQ * SA_MAXH], sA[SA_TQ * SA_MAXH];
  const int tid = threadIdx.x;
  int s0 = off[blockIdx.x], s1 = off[blockIdx.x + 1];
  if (s0 < 0) s0 = 0;
  if (s1 > R) s1 = R;
  const int L = s1 - s0;
  if (L <= 0) return;
  const int dh = d / heads, ld = 3 * d;
  const float sc = 1.0f / sqrtf((float)dh);
  for (int q0 = 0; q0 < L; q0 += SA_TQ) {
    const int nq = L - q0 < SA_TQ ? L - q0 : SA_TQ;
    __syncthreads();  // the pass before is read out
    for (int e = tid; e < nq * d; e += 256) {
      const int i = e / d, c = e - i * d;
      sQ[i][c] = qkv[(size_t)(s0 + q0 + i) * ld + c] * sc;
    }
    if (tid < SA_TQ * SA_MAXH) sM[tid] = -INFINITY, sL[tid] = 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};  // output element tid + 256 u of the pass: row (e / d), column (e % d)
    for (int k0 = 0; k0 < L; k0 += SA_T) {
      const int nk = L - k0 < SA_T ? L - k0 : SA_T;
      __syncthreads();  // the tile before is consumed
      for (int e = tid; e < nk * d; e += 256) {
        const int j = e / d, c = e - j * d;
        const float* row = qkv + (size_t)(s0 + k0 + j) * ld;
        sK[j][c] = row[d + c];
        sV[j][c] = row[2 * d + c];
      }
      __syncthreads();
      for (int e = tid; e < nq * heads * nk; e += 256) {
        const int j = e % nk, ih = e / nk, h = ih % heads, i = ih / heads;
        const float* qa = &sQ[i][h * dh];
        const float* ka = &sK[j][h * dh];
        float s = 0.f;
        for (int t = 0; t < dh; ++t) s = fmaf(qa[t], ka[t], s);
        sS[SA_S(i, h, j)] = s;
      }
      __syncthreads();
      if (tid < nq * heads) {  // running maximum and sum of (query, head); the scores become exp(score - maximum)
        const int h = tid % heads, i = tid / heads, st = i * SA_MAXH + h;
        float* srow = &sS[SA_S(i, h, 0)];
        const float m = sM[st];
        float mx = m;
        for (int j = 0; j < nk; ++j) mx = fmaxf(mx, srow[j]);
        const float a = expf(m - mx);  // (first tile: exp(-inf) = 0)
        float l = sL[st] * a;
        for (int j = 0; j < nk; ++j) {
          const float p = expf(srow[j] - mx);
          srow[j] = p;
          l += p;
        }
        sM[st] = mx, sL[st] = l, sA[st] = a;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + 256 * u;
        if (e < nq * d) {
          const int i = e / d, c = e - i * d, h = c / dh;
          const float* p = &sS[SA_S(i, h, 0)];
          float a = acc[u] * sA[i * SA_MAXH + h];
          for (int j = 0; j < nk; ++j) a = fmaf(p[j], sV[j][c], a);
          acc[u] = a;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u;
      if (e < nq * d) {
        const int i = e / d, c = e - i * d, h = c / dh;
        y[(size_t)(s0 + q0 + i) * d + c] = acc[u] / sL[i * SA_MAXH + h];
      }
    }
    if (tid < nq * heads) {
      const int h = tid % heads, i = tid / heads, st = i * SA_MAXH + h;
      lse[(size_t)(s0 + q0 + i) * heads + h] = sM[st] + logf(sL[st]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ attention backward
// P_ij = exp(score_ij - lse_i), D_i = <dy_i, y_i> per head, dS = P (dy_i . v_j - D_i):
//   dV_j = sum_i P_ij dy_i     dQ_i = sum_j dS_ij k_j / sqrt(dh)     dK_j = sum_i dS_ij q_i / sqrt(dh)
__global__ void __launch_bounds__(256) k_star_attn_bwd(const float* __restrict__ dy, const float* __restrict__ qkv,
                                                       const float* __restrict__ y, const float* __restrict__ lse,
                                                       const int32_t* __restrict__ off, int R, int d, int heads, float* __restrict__ dqkv) {
  __shared__ float sQ[SA_TQ][SA_MAXD];
  __shared__ float sG[SA_TQ][SA_MAXD];  // dy rows of the pass
  __shared__ float sK[SA_T][SA_MAXD + 1];
  __shared__ float sV[SA_T][SA_MAXD + 1];
  __shared__ float sS[SA_TQ * SA_MAXH * SA_T];  // dS
  __shared__ float sP[SA_TQ * SA_MAXH * SA_T];  // P
  __shared__ float sD[SA_TQ * SA_MAXH], sE[SA_TQ * SA_MAXH];
  const int tid = threadIdx.x;
  int s0 = off[blockIdx.x], s1 = off[blockIdx.x + 1];
  if (s0 < 0) s0 = 0;
  if (s1 > R) s1 = R;
  const int L = s1 - s0;
  if (L <= 0) return;
  const int dh = d / heads, ld = 3 * d;
  const float sc = 1.0f / sqrtf((float)dh);
  const bool for_q = blockIdx.y == 0;
  const int outer_step = for_q ? SA_TQ : SA_T;
  for (int o0 = 0; o0 < L; o0 += outer_step) {
    // for_q: o0 is a query pass, the inner loop walks key tiles; else o0 is a key tile, the inner loop walks query passes
    float accA[8], accB[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) accA[u] = accB[u] = 0.f;
    const int inner_step = for_q ? SA_T : SA_TQ;
    for (int i0 = 0; i0 < L; i0 += inner_step) {
      const int q0 = for_q ? o0 : i0, k0 = for_q ? i0 : o0;
      const int nq = L - q0 < SA_TQ ? L - q0 : SA_TQ;
      const int nk = L - k0 < SA_T ? L - k0 : SA_T;
      __syncthreads();  // the tiles before are consumed
      if (!for_q || i0 == 0) {  // query side: rows, dy, lse and D
        for (int e = tid; e < nq * d; e += 256) {
          const int i = e / d, c = e - i * d;
          sQ[i][c] = qkv[(size_t)(s0 + q0 + i) * ld + c] * sc;
          sG[i][c] = dy[(size_t)(s0 + q0 + i) * d + c];
        }
        if (tid < nq * heads) {
          const int h = tid % heads, i = tid / heads;
          const float* gy = dy + (size_t)(s0 + q0 + i) * d + h * dh;
          const float* yy = y + (size_t)(s0 + q0 + i) * d + h * dh;
          float dsum = 0.f;
          for (int t = 0; t < dh; ++t) dsum = fmaf(gy[t], yy[t], dsum);
          sD[i * SA_MAXH + h] = dsum;
          sE[i * SA_MAXH + h] = lse[(size_t)(s0 + q0 + i) * heads + h];
        }
      }
      if (for_q || i0 == 0) {  // key side
        for (int e = tid; e < nk * d; e += 256) {
          const int j = e / d, c = e - j * d;
          const float* row = qkv + (size_t)(s0 + k0 + j) * ld;
          sK[j][c] = row[d + c];
          sV[j][c] = row[2 * d + c];
        }
      }
      __syncthreads();
      for (int e = tid; e < nq * heads * nk; e += 256) {
        const int j = e % nk, ih = e / nk, h = ih % heads, i = ih / heads;
        const float* qa = &sQ[i][h * dh];
        const float* ga = &sG[i][h * dh];
        const float* ka = &sK[j][h * dh];
        const float* va = &sV[j][h * dh];
        float s = 0.f, dp = 0.f;
        for (int t = 0; t < dh; ++t) {
          s = fmaf(qa[t], ka[t], s);
          dp = fmaf(ga[t], va[t], dp);
        }
        const float p = expf(s - sE[i * SA_MAXH + h]);
        sP[SA_S(i, h, j)] = p;
        sS[SA_S(i, h, j)] = p * (dp - sD[i * SA_MAXH + h]);
      }
      __syncthreads();
      if (for_q) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = tid + 256 * u;
          if (e < nq * d) {
            const int i = e / d, c = e - i * d, h = c / dh;
            const float* ds = &sS[SA_S(i, h, 0)];
            float a = accA[u];
            for (int j = 0; j < nk; ++j) a = fmaf(ds[j], sK[j][c], a);
            accA[u] = a;
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int e = tid + 256 * u;
          if (e < nk * d) {
            const int j = e / d, c = e - j * d, h = c / dh;
            float a = accA[u], bsum = accB[u];
            for (int i = 0; i < nq; ++i) {
              a = fmaf(sS[SA_S(i, h, j)], sQ[i][c], a);     // (sQ holds q / sqrt(dh))
              bsum = fmaf(sP[SA_S(i, h, j)], sG[i][c], bsum);
            }
            accA[u] = a, accB[u] = bsum;
          }
        }
      }
    }
    if (for_q) {
      const int nq = L - o0 < SA_TQ ? L - o0 : SA_TQ;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + 256 * u;
        if (e < nq * d) {
          const int i = e / d, c = e - i * d;
          dqkv[(size_t)(s0 + o0 + i) * ld + c] = accA[u] * sc;
        }
      }
    } else {
      const int nk = L - o0 < SA_T ? L - o0 : SA_T;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = tid + 256 * u;
        if (e < nk * d) {
          const int j = e / d, c = e - j * d;
          dqkv[(size_t)(s0 + o0 + j) * ld + d + c] = accA[u];
          dqkv[(size_t)(s0 + o0 + j) * ld + 2 * d + c] = accB[u];
        }
      }
    }
  }
}

static int star_attn_args(const char* who, int64_t R, int64_t B, int d, int heads) {
  if (!star_d_ok(d)) return failf(1, who, "d must be 16, 32, 64 or 128");
  if (!(heads == 1 || heads == 2 || heads == 4 || heads == 8 || heads == 16) || d % heads != 0)
    return failf(1, who, "heads must be 1, 2, 4, 8 or 16 and divide d");
  if (R < 0 || B < 0 || B > R) return failf(1, who, "negative row or segment count, or more segments than rows");
  if (R > SA_ROW_LIMIT) return failf(1, who, "more rows than INT32_MAX / (3 * 128)");
  return 0;
}

extern "C" int mgn_star_attn_tile_rows(void) { return SA_T; }

extern "C" int mgn_star_attn_fwd(const float* qkv, const int32_t* off, int64_t R, int64_t B, int d, int heads, float* y, float* lse,
                                 void* stream) {
  if (const int rc = star_attn_args("mgn_star_attn_fwd", R, B, d, heads)) return rc;
  if (R == 0 || B == 0) return 0;
  if (qkv == nullptr || off == nullptr || y == nullptr || lse == nullptr) return fail(1, "mgn_star_attn_fwd: null pointer");
  hipLaunchKernelGGL(k_star_attn_fwd, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, qkv, off, (int)R, d, heads, y, lse);
  return check_launch("mgn_star_attn_fwd");
}

extern "C" int mgn_star_attn_bwd(const float* dy, const float* qkv, const float* y, const float* lse, const int32_t* off, int64_t R,
                                 int64_t B, int d, int heads, float* dqkv, void* stream) {
  if (const int rc = star_attn_args("mgn_star_attn_bwd", R, B, d, heads)) return rc;
  if (R == 0 || B == 0) return 0;
  if (dy == nullptr || qkv == nullptr || y == nullptr || lse == nullptr || off == nullptr || dqkv == nullptr)
    return fail(1, "mgn_star_attn_bwd: null pointer");
  hipLaunchKernelGGL(k_star_attn_bwd, dim3((unsigned)B, 2), dim3(256), 0, (hipStream_t)stream, dy, qkv, y, lse, off, (int)R, d, heads, dqkv);
  return check_launch("mgn_star_attn_bwd");
}

// ------------------------------------------------------------------------------------------------ loss tail
__global__ void __launch_bounds__(256) k_star_loss(const float* __restrict__ yhat, const float* __restrict__ target,
                                                   const int32_t* __restrict__ row_node, const int32_t* __restrict__ off, int N, int B, int R,
                                                   int O, int reduction, float* __restrict__ out, float* __restrict__ dyhat) {
  __shared__ double s_c[256], s_p[256];
  const int tid = threadIdx.x;
  const int T = R - B;
  double a_center = 0.0, a_pair = 0.0;
  for (int b = tid; b < B; b += 256) {
    const int s0 = off[b];
    int deg = off[b + 1] - s0 - 1;
    if (deg < 0 || s0 < 0 || s0 + 1 + deg > R) deg = 0;
    const float cnt = deg > 1 ? (float)deg : 1.f;
    const float w = reduction == 0 ? 2.f / ((float)O * cnt * (float)B) : 2.f / ((float)O * (float)T);
    double sb = 0.0;
    for (int t = 0; t < deg; ++t) {
      const int r = s0 + 1 + t, row = r - b - 1;
      const int node = row_node[r];
      const bool ok = node >= 0 && node < N;
      float e = 0.f;
      for (int c = 0; c < O; ++c) {
        const float dl = ok ? yhat[(size_t)row * O + c] - target[(size_t)node * O + c] : 0.f;
        e = fmaf(dl, dl, e);
        dyhat[(size_t)row * O + c] = dl * w;
      }
      sb += (double)(e / (float)O);
    }
    a_pair += sb;
    a_center += sb / (double)cnt;
  }
  s_c[tid] = a_center, s_p[tid] = a_pair;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_c[tid] += s_c[tid + o], s_p[tid] += s_p[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double pair = s_p[0] / (double)T;
    out[0] = (float)(reduction == 0 ? s_c[0] / (double)B : pair);
    out[1] = (float)pair;
  }
}

extern "C" int mgn_star_loss(const float* yhat, const float* target, const int32_t* row_node, const int32_t* off, int64_t N, int64_t B,
                             int64_t R, int O, int reduction, float* out, float* dyhat, void* stream) {
  if (O < 1 || O > 32) return fail(1, "mgn_star_loss: output width outside 1..32");
  if (reduction != 0 && reduction != 1) return fail(1, "mgn_star_loss: reduction must be 0 (mean_per_center) or 1 (mean)");
  if (N < 1 || N >= 0x7fffffff || B < 1 || R <= B || R > SA_ROW_LIMIT)
    return fail(1, "mgn_star_loss: needs at least one star and one neighbour row, and at most INT32_MAX / 384 rows");
  if (yhat == nullptr || target == nullptr || row_node == nullptr || off == nullptr || out == nullptr || dyhat == nullptr)
    return fail(1, "mgn_star_loss: null pointer");
  hipLaunchKernelGGL(k_star_loss, dim3(1), dim3(256), 0, (hipStream_t)stream, yhat, target, row_node, off, (int)N, (int)B, (int)R, O, reduction,
                     out, dyhat);
  return check_launch("mgn_star_loss");
}
