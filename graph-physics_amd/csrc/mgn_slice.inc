// The physics (slice) attention of the Transolver processor, included by mgn_attn.hip behind mgn_starattn.inc (the error channel
// and philox4x32_10 come from there); declared in include/mgn_hip_slice.h.
//
// The reference (graphphysics/models/transolver.py) works on [B, H, N, C] tensors and einsums; here the rows stay N-major and every
// step is one pass over them.  Everything is node-sized and memory-bound: the arithmetic per (row, head) is two G x C dot-product
// sets, a softmax over G and a handful of transcendental calls.
//
//   k_slice_uniforms     one thread per element of u[N, H, G]
//   k_slice_weights_fwd  one LANE per slice: a (row, head) pair owns P = the power of two >= G consecutive lanes of a wavefront, so a
//                        wavefront serves 64 / P pairs at once.  The two G x C matrices sit in LDS, transposed ([c][lane]: the lanes of
//                        a pair read consecutive words), the row's x is read as a broadcast.  Sums and the maximum over G are xor
//                        butterflies inside the P lanes: a fixed order, the same on every lane
//   k_slice_aggregate    grid (blocks, H): every workgroup walks a contiguous range of nodes in tiles of SL_AGG_TR rows staged in LDS; a
//                        thread owns up to 17 of the G * C + G outputs of its head in registers.  Partials go to the workspace,
//                        k_slice_agg_finish adds them in block order
//   k_slice_expand       grid (blocks, H): the head's G x C tokens and a tile of SL_EXP_TR rows of w in LDS, one thread per output
//   k_slice_rows_bwd     grid (blocks, H), the lane mapping of the forward; the head's tokens and dS join the two matrices in LDS.  The
//                        logits are formed again (same code, same bits) instead of being stored.  dx needs a sum over the lanes per
//                        channel: C butterflies.  dw2 / db2 / dbias partials per workgroup, k_slice_bwd_finish adds them in order
//
// No atomics; fixed orders everywhere: the same bits on every run.
#include "mgn_hip_slice.h"

#define SL_THREADS 256
#define SL_WAVES (SL_THREADS / 64)
#define SL_MAX_G 64
#define SL_MAX_C 64
#define SL_MAX_H 65535
#define SL_MAX_LAYER 4096
#define SL_FWD_MAX_BLOCKS 1024   // k_slice_weights_fwd
#define SL_BWD_MAX_BLOCKS 512    // k_slice_rows_bwd (per head)
#define SL_AGG_TR 32             // rows per LDS tile of k_slice_aggregate
#define SL_AGG_MAX_BLOCKS 1024   // over all heads: 1024 / H per head (128 at 8 heads; the one-"head" weight-gradient form gets them all)
#define SL_AGG_KMAX 17           // outputs per thread: 64 * 64 + 64 = 16.25 * 256
#define SL_EXP_TR 64             // rows per LDS tile of k_slice_expand
#define SL_EXP_MAX_BLOCKS 1024   // (per head)
#define SL_TAG 0x534c4943u

static_assert(SL_MAX_G * SL_MAX_C + SL_MAX_G <= SL_AGG_KMAX * SL_THREADS, "k_slice_aggregate: every output needs an owner");
static_assert(4 * SL_MAX_G * SL_MAX_C * sizeof(float) <= 65536, "k_slice_rows_bwd keeps four G x C matrices in LDS");

static inline int sl_pow2(int G) {
  int p = 1;
  while (p < G) p <<= 1;
  return p;
}

__device__ __forceinline__ float sl_uniform(uint32_t k0, uint32_t k1, int64_t row, int g, int layer, int64_t step) {
  uint32_t r0, r1;
  philox4x32_10(k0, k1, (uint32_t)row, (uint32_t)(g >> 1) | ((uint32_t)layer << 8) | ((uint32_t)((uint64_t)row >> 32) << 20), (uint32_t)step,
                (uint32_t)((uint64_t)step >> 32) ^ SL_TAG, r0, r1);
  return (float)(((g & 1) ? r1 : r0) >> 8) * 5.9604644775390625e-08f;
}

__device__ __forceinline__ float sl_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float sl_gelu_grad(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}
__device__ __forceinline__ float sl_gumbel(float u) { return -logf(-logf(u + 1e-8f) + 1e-8f); }

// sum / maximum over the P consecutive lanes of a (row, head) pair: every lane ends with the same value
__device__ __forceinline__ float sl_gsum(float v, int P) {
  for (int m = P >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float sl_gmax(float v, int P) {
  for (int m = P >> 1; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

static int sl_sizes_ok(const char* who, int64_t N, int H, int G, int C, int layer) {
  if (G < 1 || G > SL_MAX_G) return failf(1, who, "slice_num must be in 1..64");
  if (C < 1 || C > SL_MAX_C) return failf(1, who, "channels per head must be in 1..64");
  if (H < 1 || H > SL_MAX_H) return failf(1, who, "heads must be in 1..65535");
  if (layer < 0 || layer >= SL_MAX_LAYER) return failf(1, who, "layer must be in 0..4095");
  if (N < 0 || N > (((int64_t)1 << 44) - 1) / H) return failf(1, who, "row count out of range");
  return 0;
}

extern "C" int64_t mgn_slice_pass_rows(int launch, int G) {
  if (G < 1 || G > SL_MAX_G) return 0;
  const int64_t rpb = (int64_t)SL_WAVES * (64 / sl_pow2(G));
  switch (launch) {
    case 2: return rpb * SL_FWD_MAX_BLOCKS;
    case 3: return (int64_t)SL_AGG_TR * SL_AGG_MAX_BLOCKS;
    case 4: return (int64_t)SL_EXP_TR * SL_EXP_MAX_BLOCKS;
    case 5: return rpb * SL_BWD_MAX_BLOCKS;
    default: return 0;
  }
}

// ------------------------------------------------------------------------------------------------ 1: uniforms
__global__ void __launch_bounds__(SL_THREADS) k_slice_uniforms(uint32_t k0, uint32_t k1, const int64_t* __restrict__ step_ptr, int layer, int64_t total,
                                                               int G, float* __restrict__ u) {
  const int64_t step = step_ptr ? *step_ptr : 0;
  for (int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * SL_THREADS) {
    const int64_t row = i / G;
    u[i] = sl_uniform(k0, k1, row, (int)(i - row * G), layer, step);
  }
}

extern "C" int mgn_slice_uniforms(uint64_t seed, const int64_t* step, int layer, int64_t N, int H, int G, float* u, void* stream) {
  if (sl_sizes_ok("mgn_slice_uniforms", N, H, G, 1, layer)) return 1;
  if (N > 0 && u == nullptr) return fail(1, "mgn_slice_uniforms: null pointer");
  if (N == 0) return 0;
  const int64_t total = N * H * G;
  const int64_t nb = (total + SL_THREADS - 1) / SL_THREADS;
  hipLaunchKernelGGL(k_slice_uniforms, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(SL_THREADS), 0, (hipStream_t)stream, (uint32_t)seed,
                     (uint32_t)(seed >> 32), step, layer, total, G, u);
  return check_launch("mgn_slice_uniforms");
}

// ------------------------------------------------------------------------------------------------ 2: slice weights
// what forward and backward both form for one lane of a (row, head) pair: the logit a + gum and the temperature layer's pre-activation
__device__ __forceinline__ void sl_lane_dots(const float* __restrict__ xp, const float* sWs, const float* sW1, int C, int P, int g, float bs, float b1,
                                             float& a, float& p1) {
  a = bs, p1 = b1;
  for (int c = 0; c < C; ++c) {
    const float xv = xp[c];
    a = fmaf(sWs[c * P + g], xv, a);
    p1 = fmaf(sW1[c * P + g], xv, p1);
  }
}

__global__ void __launch_bounds__(SL_THREADS) k_slice_weights_fwd(const float* __restrict__ x, int64_t ldx, const float* __restrict__ Ws,
                                                                  const float* __restrict__ bs, const float* __restrict__ W1,
                                                                  const float* __restrict__ b1, const float* __restrict__ w2,
                                                                  const float* __restrict__ b2, const float* __restrict__ bias,
                                                                  const float* __restrict__ u_in, uint32_t k0, uint32_t k1,
                                                                  const int64_t* __restrict__ step_ptr, int layer, int64_t NR, int H, int G, int C,
                                                                  int P, float* __restrict__ w_out, float* __restrict__ rowsc) {
  extern __shared__ float sl_sm[];
  float* sWs = sl_sm;
  float* sW1 = sl_sm + C * P;
  const int tid = threadIdx.x;
  for (int i = tid; i < C * P; i += SL_THREADS) {
    const int c = i / P, g = i - c * P;
    sWs[i] = g < G ? Ws[g * C + c] : 0.0f;
    sW1[i] = g < G ? W1[g * C + c] : 0.0f;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, g = lane & (P - 1), sub = lane / P, rpw = 64 / P, rpb = SL_WAVES * rpw;
  const bool act = g < G;
  const float my_bs = act ? bs[g] : 0.0f, my_b1 = act ? b1[g] : 0.0f, my_w2 = act ? w2[g] : 0.0f, b2v = b2[0];
  const int64_t step = step_ptr ? *step_ptr : 0;
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < NR; base += (int64_t)gridDim.x * rpb) {
    const int64_t r = base + wave * rpw + sub;
    const bool valid = r < NR;
    const int64_t rr = valid ? r : 0;
    const int64_t n = rr / H;
    const int h = (int)(rr - n * H);
    float a, p1;
    sl_lane_dots(x + n * ldx + (int64_t)h * C, sWs, sW1, C, P, g, my_bs, my_b1, a, p1);
    const float t2 = sl_gsum(my_w2 * sl_gelu(p1), P) + b2v;
    const float tpre = sl_gelu(t2) + bias[h];
    const float t = fmaxf(tpre, 0.01f);
    const float u = !act ? 0.5f : (u_in ? u_in[rr * G + g] : sl_uniform(k0, k1, rr, g, layer, step));
    // softmax((y - c) / t) with c = the row maximum of y: the same function for any c; the maximum goes before the division, so the
    // exponent's argument comes from small operands (and the backward's temperature gradient, formed the same way, does not cancel)
    const float y = a + sl_gumbel(u);
    const float ym = sl_gmax(act ? y : -INFINITY, P);
    const float e = act ? expf((y - ym) / t) : 0.0f;
    const float s = sl_gsum(e, P);
    if (valid && act) w_out[rr * G + g] = e / s;
    if (valid && g == 0) rowsc[2 * rr] = t2, rowsc[2 * rr + 1] = tpre;
  }
}

extern "C" int mgn_slice_weights_fwd(const float* x_mid, int64_t ldx, const float* Ws, const float* bs, const float* W1, const float* b1,
                                     const float* w2, const float* b2, const float* bias, const float* u, uint64_t seed, const int64_t* step,
                                     int layer, int64_t N, int H, int G, int C, float* w, float* rowsc, void* stream) {
  if (sl_sizes_ok("mgn_slice_weights_fwd", N, H, G, C, layer)) return 1;
  if (!Ws || !bs || !W1 || !b1 || !w2 || !b2 || !bias || (N > 0 && (!x_mid || !w || !rowsc)))
    return fail(1, "mgn_slice_weights_fwd: null pointer");
  if (ldx < (int64_t)H * C) return fail(1, "mgn_slice_weights_fwd: leading dimension below heads * channels");
  if (N == 0) return 0;
  const int P = sl_pow2(G), rpb = SL_WAVES * (64 / P);
  const int64_t NR = N * H, nb = (NR + rpb - 1) / rpb;
  hipLaunchKernelGGL(k_slice_weights_fwd, dim3((unsigned)(nb < SL_FWD_MAX_BLOCKS ? nb : SL_FWD_MAX_BLOCKS)), dim3(SL_THREADS),
                     (size_t)2 * C * P * sizeof(float), (hipStream_t)stream, x_mid, ldx, Ws, bs, W1, b1, w2, b2, bias, u, (uint32_t)seed,
                     (uint32_t)(seed >> 32), step, layer, NR, H, G, C, P, w, rowsc);
  return check_launch("mgn_slice_weights_fwd");
}

// ------------------------------------------------------------------------------------------------ 3: reduction over the nodes
static inline int sl_agg_blocks(int64_t N, int H) {
  const int64_t nb = (N + 255) / 256;
  const int cap = SL_AGG_MAX_BLOCKS / H > 1 ? SL_AGG_MAX_BLOCKS / H : 1;
  return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

__global__ void __launch_bounds__(SL_THREADS) k_slice_aggregate(const float* __restrict__ w, const float* __restrict__ x, int64_t ldx, int64_t N, int H,
                                                                int G, int C, float* __restrict__ part) {
  __shared__ float sw[SL_AGG_TR * SL_MAX_G];
  __shared__ float sx[SL_AGG_TR * SL_MAX_C];
  const int tid = threadIdx.x, h = blockIdx.y, nbx = gridDim.x, nout = G * C + G;
  const int64_t chunk = (N + nbx - 1) / nbx;
  const int64_t n0 = (int64_t)blockIdx.x * chunk;
  const int64_t n1 = n0 + chunk < N ? n0 + chunk : N;
  float acc[SL_AGG_KMAX];
#pragma unroll
  for (int k = 0; k < SL_AGG_KMAX; ++k) acc[k] = 0.0f;
  for (int64_t t0 = n0; t0 < n1; t0 += SL_AGG_TR) {
    const int rows = (int)(n1 - t0 < SL_AGG_TR ? n1 - t0 : SL_AGG_TR);
    for (int i = tid; i < rows * G; i += SL_THREADS) {
      const int r = i / G, g = i - r * G;
      sw[i] = w[((t0 + r) * H + h) * G + g];
    }
    for (int i = tid; i < rows * C; i += SL_THREADS) {
      const int r = i / C, c = i - r * C;
      sx[i] = x[(t0 + r) * ldx + (int64_t)h * C + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SL_AGG_KMAX; ++k) {
      const int o = tid + k * SL_THREADS;
      if (o < G * C) {
        const int g = o / C, c = o - g * C;
        float s = acc[k];
        for (int r = 0; r < rows; ++r) s = fmaf(sw[r * G + g], sx[r * C + c], s);
        acc[k] = s;
      } else if (o < nout) {
        const int g = o - G * C;
        float s = acc[k];
        for (int r = 0; r < rows; ++r) s += sw[r * G + g];
        acc[k] = s;
      }
    }
    __syncthreads();
  }
  float* dst = part + ((int64_t)h * nbx + blockIdx.x) * nout;
#pragma unroll
  for (int k = 0; k < SL_AGG_KMAX; ++k) {
    const int o = tid + k * SL_THREADS;
    if (o < nout) dst[o] = acc[k];
  }
}

__global__ void __launch_bounds__(SL_THREADS) k_slice_agg_finish(const float* __restrict__ part, int nbx, int H, int G, int C, float* __restrict__ S,
                                                                 float* __restrict__ norm) {
  const int nout = G * C + G;
  const int64_t i = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (i >= (int64_t)H * nout) return;
  const int h = (int)(i / nout), o = (int)(i - (int64_t)h * nout);
  const float* p = part + (int64_t)h * nbx * nout + o;
  float s = 0.0f;
  for (int b = 0; b < nbx; ++b) s += p[(int64_t)b * nout];
  if (o < G * C)
    S[(int64_t)h * G * C + o] = s;
  else if (norm)
    norm[(int64_t)h * G + (o - G * C)] = s;
}

extern "C" size_t mgn_slice_aggregate_workspace_bytes(int64_t N, int H, int G, int C) {
  if (N < 0 || H < 1 || G < 1 || G > SL_MAX_G || C < 1 || C > SL_MAX_C) return 0;
  return (size_t)H * sl_agg_blocks(N, H) * ((size_t)G * C + G) * sizeof(float) + 256;
}

extern "C" int mgn_slice_aggregate(const float* w, const float* x, int64_t ldx, int64_t N, int H, int G, int C, float* S, float* norm, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (sl_sizes_ok("mgn_slice_aggregate", N, H, G, C, 0)) return 1;
  if (!S || (N > 0 && (!w || !x))) return fail(1, "mgn_slice_aggregate: null pointer");
  if (ldx < (int64_t)H * C) return fail(1, "mgn_slice_aggregate: leading dimension below heads * channels");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    if (hipMemsetAsync(S, 0, (size_t)H * G * C * sizeof(float), s) != hipSuccess) return fail(2, "mgn_slice_aggregate: memset");
    if (norm && hipMemsetAsync(norm, 0, (size_t)H * G * sizeof(float), s) != hipSuccess) return fail(2, "mgn_slice_aggregate: memset");
    return 0;
  }
  const int nbx = sl_agg_blocks(N, H);
  const size_t need = (size_t)H * nbx * ((size_t)G * C + G) * sizeof(float);
  float* part = (float*)ws_base(ws, ws_bytes, need);
  if (part == nullptr) return fail(1, "mgn_slice_aggregate: workspace too small (mgn_slice_aggregate_workspace_bytes)");
  hipLaunchKernelGGL(k_slice_aggregate, dim3(nbx, H), dim3(SL_THREADS), 0, s, w, x, ldx, N, H, G, C, part);
  const int64_t outs = (int64_t)H * (G * C + G);
  hipLaunchKernelGGL(k_slice_agg_finish, dim3((unsigned)((outs + SL_THREADS - 1) / SL_THREADS)), dim3(SL_THREADS), 0, s, part, nbx, H, G, C, S, norm);
  return check_launch("mgn_slice_aggregate");
}

// ------------------------------------------------------------------------------------------------ 4: broadcast back to the rows
__global__ void __launch_bounds__(SL_THREADS) k_slice_expand(const float* __restrict__ w, const float* __restrict__ tok, int64_t N, int H, int G, int C,
                                                             float* __restrict__ out, int64_t ldo) {
  __shared__ float stok[SL_MAX_G * SL_MAX_C];
  __shared__ float sw[SL_EXP_TR * SL_MAX_G];
  const int tid = threadIdx.x, h = blockIdx.y;
  for (int i = tid; i < G * C; i += SL_THREADS) stok[i] = tok[(int64_t)h * G * C + i];
  for (int64_t t0 = (int64_t)blockIdx.x * SL_EXP_TR; t0 < N; t0 += (int64_t)gridDim.x * SL_EXP_TR) {
    const int rows = (int)(N - t0 < SL_EXP_TR ? N - t0 : SL_EXP_TR);
    __syncthreads();
    for (int i = tid; i < rows * G; i += SL_THREADS) {
      const int r = i / G, g = i - r * G;
      sw[i] = w[((t0 + r) * H + h) * G + g];
    }
    __syncthreads();
    for (int i = tid; i < rows * C; i += SL_THREADS) {
      const int r = i / C, c = i - r * C;
      float s = 0.0f;
      for (int g = 0; g < G; ++g) s = fmaf(sw[r * G + g], stok[g * C + c], s);
      out[(t0 + r) * ldo + (int64_t)h * C + c] = s;
    }
  }
}

extern "C" int mgn_slice_expand(const float* w, const float* tok, int64_t N, int H, int G, int C, float* out, int64_t ldo, void* stream) {
  if (sl_sizes_ok("mgn_slice_expand", N, H, G, C, 0)) return 1;
  if (!tok || (N > 0 && (!w || !out))) return fail(1, "mgn_slice_expand: null pointer");
  if (ldo < (int64_t)H * C) return fail(1, "mgn_slice_expand: leading dimension below heads * channels");
  if (N == 0) return 0;
  const int64_t nb = (N + SL_EXP_TR - 1) / SL_EXP_TR;
  hipLaunchKernelGGL(k_slice_expand, dim3((unsigned)(nb < SL_EXP_MAX_BLOCKS ? nb : SL_EXP_MAX_BLOCKS), H), dim3(SL_THREADS), 0, (hipStream_t)stream, w,
                     tok, N, H, G, C, out, ldo);
  return check_launch("mgn_slice_expand");
}

// ------------------------------------------------------------------------------------------------ 5: per-row backward
static inline int sl_bwd_blocks(int64_t N, int G) {
  const int rpb = SL_WAVES * (64 / sl_pow2(G));
  const int64_t nb = (N + rpb - 1) / rpb;
  return (int)(nb < 1 ? 1 : (nb > SL_BWD_MAX_BLOCKS ? SL_BWD_MAX_BLOCKS : nb));
}

__global__ void __launch_bounds__(SL_THREADS) k_slice_rows_bwd(const float* __restrict__ dOut, int64_t lddo, const float* __restrict__ tok,
                                                               const float* __restrict__ dS, const float* __restrict__ dnorm,
                                                               const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                               const float* __restrict__ rowsc, const float* __restrict__ Ws,
                                                               const float* __restrict__ bs, const float* __restrict__ W1,
                                                               const float* __restrict__ b1, const float* __restrict__ w2,
                                                               const float* __restrict__ u_in, uint32_t k0, uint32_t k1,
                                                               const int64_t* __restrict__ step_ptr, int layer, int64_t N, int H, int G, int C, int P,
                                                               float* __restrict__ dx, int64_t lddx, float* __restrict__ da, float* __restrict__ dh1,
                                                               float* __restrict__ dt2_out, float* __restrict__ part) {
  extern __shared__ float sl_sm[];   // four [C][P] matrices; at the end the first 3 * SL_THREADS floats hold the workgroup's partial sums
  const int CP = C * P;
  float* sWs = sl_sm;
  float* sW1 = sl_sm + CP;
  float* sTok = sl_sm + 2 * CP;
  float* sdS = sl_sm + 3 * CP;
  const int tid = threadIdx.x, h = blockIdx.y;
  for (int i = tid; i < CP; i += SL_THREADS) {
    const int c = i / P, g = i - c * P;
    const bool in = g < G;
    sWs[i] = in ? Ws[g * C + c] : 0.0f;
    sW1[i] = in ? W1[g * C + c] : 0.0f;
    sTok[i] = in ? tok[((int64_t)h * G + g) * C + c] : 0.0f;
    sdS[i] = in ? dS[((int64_t)h * G + g) * C + c] : 0.0f;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, g = lane & (P - 1), sub = lane / P, rpw = 64 / P, rpb = SL_WAVES * rpw;
  const bool act = g < G;
  const float my_bs = act ? bs[g] : 0.0f, my_b1 = act ? b1[g] : 0.0f, my_w2 = act ? w2[g] : 0.0f;
  const float my_dn = act ? dnorm[(int64_t)h * G + g] : 0.0f;
  const int64_t step = step_ptr ? *step_ptr : 0;
  float acc_w2 = 0.0f, acc_b2 = 0.0f, acc_bias = 0.0f;
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < N; base += (int64_t)gridDim.x * rpb) {
    const int64_t n_ = base + wave * rpw + sub;
    const bool valid = n_ < N;
    const int64_t n = valid ? n_ : 0;
    const int64_t r = n * H + h;
    const float* xp = x + n * ldx + (int64_t)h * C;
    const float* dop = dOut + n * lddo + (int64_t)h * C;
    float a, p1;
    sl_lane_dots(xp, sWs, sW1, C, P, g, my_bs, my_b1, a, p1);
    float dw = my_dn;
    for (int c = 0; c < C; ++c) dw = fmaf(sdS[c * P + g], xp[c], fmaf(sTok[c * P + g], dop[c], dw));
    const float t2 = rowsc[2 * r], tpre = rowsc[2 * r + 1];
    const float t = fmaxf(tpre, 0.01f);
    const bool live = valid && act;
    const float wv = live ? w[r * G + g] : 0.0f;
    const float u = !act ? 0.5f : (u_in ? u_in[r * G + g] : sl_uniform(k0, k1, r, g, layer, step));
    const float y = a + sl_gumbel(u);
    const float sdot = sl_gsum(wv * dw, P);
    const float dz = wv * (dw - sdot);
    const float dav = dz / t;
    // sum_g dz_g = 0: any per-row constant may be taken off y; with the row maximum the terms are small and the sum does not cancel
    const float ym = sl_gmax(act ? y : -INFINITY, P);
    const float dtc = -sl_gsum(live ? dz * (y - ym) : 0.0f, P) / (t * t);
    const float dtp = (valid && tpre >= 0.01f) ? dtc : 0.0f;
    const float d2 = dtp * sl_gelu_grad(t2);
    const float dp1 = live ? d2 * my_w2 * sl_gelu_grad(p1) : 0.0f;
    if (live) {
      da[r * G + g] = dav;
      dh1[r * G + g] = dp1;
      acc_w2 = fmaf(d2, sl_gelu(p1), acc_w2);
    }
    if (valid && g == 0) {
      dt2_out[r] = d2;
      acc_b2 += d2;
      acc_bias += dtp;
    }
    float* dxp = dx + n * lddx + (int64_t)h * C;
    for (int c = 0; c < C; ++c) {
      const float v = sl_gsum(fmaf(wv, sdS[c * P + g], fmaf(sWs[c * P + g], dav, sW1[c * P + g] * dp1)), P);
      if (valid && g == (c & (P - 1))) dxp[c] = v;
    }
  }
  __syncthreads();   // the matrices are dead: their LDS takes the partial sums
  sl_sm[tid] = acc_w2, sl_sm[SL_THREADS + tid] = acc_b2, sl_sm[2 * SL_THREADS + tid] = acc_bias;
  __syncthreads();
  if (tid < G + 2) {
    const int col = tid < G ? tid : 0;
    const float* src = sl_sm + (tid < G ? 0 : (tid == G ? SL_THREADS : 2 * SL_THREADS));
    float s = 0.0f;
    for (int wv_ = 0; wv_ < SL_WAVES; ++wv_)
      for (int sb = 0; sb < rpw; ++sb) s += src[wv_ * 64 + sb * P + col];
    part[((int64_t)h * gridDim.x + blockIdx.x) * (G + 2) + tid] = s;
  }
}

// one workgroup: first every (head, column) adds its workgroups' partials in block order (into block 0's slot), then the heads are added
__global__ void __launch_bounds__(SL_THREADS) k_slice_bwd_finish(float* __restrict__ part, int nbx, int H, int G, float* __restrict__ dw2,
                                                                 float* __restrict__ db2, float* __restrict__ dbias) {
  const int nc = G + 2;
  for (int i = threadIdx.x; i < H * nc; i += SL_THREADS) {
    const int h = i / nc, j = i - h * nc;
    float* p = part + (int64_t)h * nbx * nc + j;
    float s = 0.0f;
    for (int b = 0; b < nbx; ++b) s += p[(int64_t)b * nc];
    p[0] = s;
    if (j == G + 1) dbias[h] = s;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < G + 1; j += SL_THREADS) {
    float s = 0.0f;
    for (int h = 0; h < H; ++h) s += part[(int64_t)h * nbx * nc + j];
    if (j < G)
      dw2[j] = s;
    else
      db2[0] = s;
  }
}

extern "C" size_t mgn_slice_rows_bwd_workspace_bytes(int64_t N, int H, int G) {
  if (N < 0 || H < 1 || G < 1 || G > SL_MAX_G) return 0;
  return (size_t)H * sl_bwd_blocks(N, G) * (G + 2) * sizeof(float) + 256;
}

extern "C" int mgn_slice_rows_bwd(const float* dOut, int64_t lddo, const float* tok, const float* dS, const float* dnorm, const float* x_mid,
                                  int64_t ldx, const float* w, const float* rowsc, const float* Ws, const float* bs, const float* W1,
                                  const float* b1, const float* w2, const float* u, uint64_t seed, const int64_t* step, int layer, int64_t N,
                                  int H, int G, int C, float* dx, int64_t lddx, float* da, float* dh1, float* dt2, float* dw2, float* db2,
                                  float* dbias, void* ws, size_t ws_bytes, void* stream) {
  if (sl_sizes_ok("mgn_slice_rows_bwd", N, H, G, C, layer)) return 1;
  // (the row-sized operands of an empty call may be null: an empty tensor has no address)
  if (!tok || !dS || !dnorm || !Ws || !bs || !W1 || !b1 || !w2 || !dw2 || !db2 || !dbias ||
      (N > 0 && (!dOut || !x_mid || !w || !rowsc || !dx || !da || !dh1 || !dt2)))
    return fail(1, "mgn_slice_rows_bwd: null pointer");
  if (ldx < (int64_t)H * C || lddo < (int64_t)H * C || lddx < (int64_t)H * C)
    return fail(1, "mgn_slice_rows_bwd: leading dimension below heads * channels");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    if (hipMemsetAsync(dw2, 0, (size_t)G * sizeof(float), s) != hipSuccess || hipMemsetAsync(db2, 0, sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(dbias, 0, (size_t)H * sizeof(float), s) != hipSuccess)
      return fail(2, "mgn_slice_rows_bwd: memset");
    return 0;
  }
  const int P = sl_pow2(G), nbx = sl_bwd_blocks(N, G);
  const size_t need = (size_t)H * nbx * (G + 2) * sizeof(float);
  float* part = (float*)ws_base(ws, ws_bytes, need);
  if (part == nullptr) return fail(1, "mgn_slice_rows_bwd: workspace too small (mgn_slice_rows_bwd_workspace_bytes)");
  size_t lds = (size_t)4 * C * P * sizeof(float);
  if (lds < 3 * SL_THREADS * sizeof(float)) lds = 3 * SL_THREADS * sizeof(float);
  hipLaunchKernelGGL(k_slice_rows_bwd, dim3(nbx, H), dim3(SL_THREADS), lds, s, dOut, lddo, tok, dS, dnorm, x_mid, ldx, w, rowsc, Ws, bs, W1, b1, w2,
                     u, (uint32_t)seed, (uint32_t)(seed >> 32), step, layer, N, H, G, C, P, dx, lddx, da, dh1, dt2, part);
  hipLaunchKernelGGL(k_slice_bwd_finish, dim3(1), dim3(SL_THREADS), 0, s, part, nbx, H, G, dw2, db2, dbias);
  return check_launch("mgn_slice_rows_bwd");
}
