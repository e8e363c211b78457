// Split-bf16 ("x6") generation of the H = 128 MLP kernels.  Included by mgn_kernels.hip.
//
// fp32 MFMA runs at the fp32 vector rate (157 TF/s) -- 1/16 of the bf16 matrix rate.  Here
// every fp32 operand is split into three bf16 pieces  x = x1 + x2 + x3  (8 + 8 + 8 mantissa
// bits, round-to-nearest at each step, each remainder exact in fp32) and a product is
// evaluated as the six terms of order <= 2^-16
//     x.w ~= x1w1 + x1w2 + x2w1 + x2w2 + x1w3 + x3w1        (dropped terms <= 2^-24 relative)
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: 6 MFMAs of 16 cycles replace
// 8 fp32 MFMAs of 32 cycles -- 2.67x the matrix rate at fp32-grade accuracy (the parity tests
// hold the same 1e-5 forward tolerance as the exact-fp32 kernels).
//
// Layouts.  The 16x16x32 C/D layout equals the 16x16x4 one, so the T-layout chain survives:
// lane (c,g) of an accumulator block ib holds features 16*ib + 4g + {0..3} of row c.  Two
// blocks (2j, 2j+1) packed to bf16 ARE the B operand of K-slice j (K = 32): element i of the
// lane's 8 bf16 is feature 32j + 16*(i>>2) + 4g + (i&3).  Which feature sits at which k is
// free as long as A agrees -- the weights are pre-packed (mgn_wpack) into exactly that order:
//   packed unit (one 128x128 block) = [j 0..3][piece 0..2][ob 0..7][lane 0..63][8 bf16]
//   with A element i of lane (c,g) = W[16*ob + c][32j + 16*(i>>2) + 4g + (i&3)],
// 24 KB per K-slice ("quarter"), 96 KB per unit.  A quarter is a LINEAR 24 KB copy into LDS
// (LDS-DMA, lane-linear destination) and every A fragment is one conflict-free ds_read_b128.
// LDS: ring of 3 quarters (72 KB) + constants => two workgroups per CU.

typedef unsigned u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) const u32x4 lds_cu32x4;

#define X6_QBYTES 24576
#define X6_RING 3
#define X6_FWD_LDS_BYTES(NW) (((NW) == 8 ? 6 : 3) * X6_QBYTES + 5 * 512)
#define X6_MAX_UNITS 8

#define MFMA_BF(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, (a)), __builtin_bit_cast(bf16x8, (b)), (c), 0, 0, 0)

// {bf16(a) | bf16(b) << 16}, round to nearest even (v_cvt_pk_bf16_f32)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 pk_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(u32, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf_lo(u32 q) { return __builtin_bit_cast(float, q << 16); }
__device__ __forceinline__ float bf_hi(u32 q) { return __builtin_bit_cast(float, q & 0xffff0000u); }

// two fp32 -> their three packed bf16 pieces
__device__ __forceinline__ void split2(float a, float b, u32& q1, u32& q2, u32& q3) {
  q1 = pk_bf16(a, b);
  const float ra = a - bf_lo(q1), rb = b - bf_hi(q1);  // exact
  q2 = pk_bf16(ra, rb);
  const float sa = ra - bf_lo(q2), sb = rb - bf_hi(q2);  // exact
  q3 = pk_bf16(sa, sb);
}

// a 16-row x 128 tile in T-layout (8 blocks of f32x4) -> B operands xs[j][piece].
// Written level by level over all 16 value pairs: the 7-deep dependent chain of one pair
// (cvt, shift, sub, cvt, shift, sub, cvt) would otherwise be executed pair after pair,
// latency-bound (measured ~2000 cycles per tile against ~450 issue cycles).
// TERMS == 1 (bf16 matrix mode): only the leading piece is made and used.
// [r4] The remainders x - bf16(x) come from the MATRIX pipe.  With S0 / S1 = minus the selector of
// a K-slice's first / second 16 features (an A operand of -1.0 and 0.0: lane (c, g) holds -1 at element i where
// 16 (i >> 2) + 4 g + (i & 3) == c [+ 16]), S . piece + x is ONE MFMA per 16 x 16 block, exact (one non-zero product per
// output, the sum is representable) and already in the T-layout: 12 conversions + 4 MFMAs per K-slice instead of 44 VALU
// instructions (shift / mask / two subtractions per value pair).  Same pieces bit for bit.
struct SplitSel {
  u32x4 s0, s1;
};
// (KEEP = false: re-made at every use -- ~16 VALU instructions -- instead of 8 registers held across the kernel: the chain
// kernels sit at 228-254 registers)
template <bool KEEP = false>
__device__ __forceinline__ SplitSel split_sel() {
  int lane = threadIdx.x & 63;
  if (!KEEP) asm volatile("" : "+v"(lane));  // opaque: not hoisted out of the tile loop
  const int c = lane & 15, g = lane >> 4;
  SplitSel S;
  const u32 m1 = 0xbf80u;  // bf16(-1.0)
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    // dword d holds elements i = 2d (low half), 2d + 1 (high half); element i <-> feature 16 (i >> 2) + 4 g + (i & 3)
    u32 w0 = 0, w1 = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = 2 * d + h;
      const int f = 16 * (i >> 2) + 4 * g + (i & 3);
      if (f == c) w0 |= m1 << (16 * h);
      if (f == c + 16) w1 |= m1 << (16 * h);
    }
    S.s0[d] = w0, S.s1[d] = w1;
  }
  return S;
}
__device__ __forceinline__ void split_pair_mfma(const f32x4& b0, const f32x4& b1, u32x4 (&x)[3], const SplitSel& S) {
  x[0][0] = pk_bf16(b0[0], b0[1]), x[0][1] = pk_bf16(b0[2], b0[3]);
  x[0][2] = pk_bf16(b1[0], b1[1]), x[0][3] = pk_bf16(b1[2], b1[3]);
  const f32x4 r0 = MFMA_BF(S.s0, x[0], b0), r1 = MFMA_BF(S.s1, x[0], b1);
  x[1][0] = pk_bf16(r0[0], r0[1]), x[1][1] = pk_bf16(r0[2], r0[3]);
  x[1][2] = pk_bf16(r1[0], r1[1]), x[1][3] = pk_bf16(r1[2], r1[3]);
  const f32x4 t0 = MFMA_BF(S.s0, x[1], r0), t1 = MFMA_BF(S.s1, x[1], r1);
  x[2][0] = pk_bf16(t0[0], t0[1]), x[2][1] = pk_bf16(t0[2], t0[3]);
  x[2][2] = pk_bf16(t1[0], t1[1]), x[2][3] = pk_bf16(t1[2], t1[3]);
}

template <int TERMS, bool MF = true>
__device__ __forceinline__ void split_tile(const f32x4 (&v)[8], u32x4 (&xs)[4][3]) {
  if (TERMS != 1 && MF) {  // (MF = false: instances that would spill with the MFMA form's longer-lived remainders)
    const SplitSel S = split_sel();
#pragma unroll
    for (int j = 0; j < 4; ++j) split_pair_mfma(v[2 * j], v[2 * j + 1], xs[j], S);
    return;
  }
  u32 q1[16], q2[16], q3[16];
  float ra[16], rb[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) q1[i] = pk_bf16(v[i >> 1][2 * (i & 1)], v[i >> 1][2 * (i & 1) + 1]);
  if (TERMS == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int d = 0; d < 4; ++d) xs[j][0][d] = q1[4 * j + d];
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ra[i] = v[i >> 1][2 * (i & 1)] - bf_lo(q1[i]);
    rb[i] = v[i >> 1][2 * (i & 1) + 1] - bf_hi(q1[i]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) q2[i] = pk_bf16(ra[i], rb[i]);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ra[i] -= bf_lo(q2[i]);
    rb[i] -= bf_hi(q2[i]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) q3[i] = pk_bf16(ra[i], rb[i]);
  // pair i = block i>>1, half i&1; operand of K-slice j: dwords {2j:0, 2j:1, 2j+1:0, 2j+1:1}
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      xs[j][0][d] = q1[4 * j + d];
      xs[j][1][d] = q2[4 * j + d];
      xs[j][2][d] = q3[4 * j + d];
    }
}

// ------------------------------------------------------------------ weight packing
struct WpackLaunch {
  mgn_wpack_block b[TB_MAX];
};
// one thread per (j, ob, lane) of one block: 8 weights -> 3 x 16 bytes
__global__ void __launch_bounds__(256) k_wpack(const WpackLaunch T) {
  const mgn_wpack_block B = T.b[blockIdx.y];
  const int t = blockIdx.x * 256 + threadIdx.x;  // 0 .. 2047
  const int lane = t & 63, ob = (t >> 6) & 7, j = t >> 9;
  const int c = lane & 15, g = lane >> 4;
  const int o = 16 * ob + c;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int f = 32 * j + 16 * (i >> 2) + 4 * g + (i & 3);
    v[i] = B.transpose ? B.src[(size_t)f * B.ld_src + o] : B.src[(size_t)o * B.ld_src + f];
  }
  u32x4 p1, p2, p3;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    u32 q1, q2, q3;
    split2(v[2 * h], v[2 * h + 1], q1, q2, q3);
    p1[h] = q1, p2[h] = q2, p3[h] = q3;
  }
  u32x4* dst = (u32x4*)((char*)B.dst + (size_t)j * X6_QBYTES) + ob * 64 + lane;
  dst[0] = p1;
  dst[512] = p2;   // + 8192 bytes
  dst[1024] = p3;  // + 16384 bytes
}

// ------------------------------------------------------------------ quarter GEMM
// One K-slice (32 input features) of one unit: acc[ob] += W[ob-block, slice] . x, all 8 output
// blocks, 6 terms each = 48 MFMAs.  A fragments of the NEXT output-block pair are read from LDS
// while the current pair multiplies; consecutive MFMAs alternate between two accumulators.
// `job`: LDS-DMA of a later quarter of the stream, 6 x 1 KB per wave, issued in steps 0..2;
// `late(s)`: the caller's operand prefetch, two loads per step -- a burst of 16 loads stalls the
// issuing wave for ~1.5 us on VMEM back-pressure (s_memrealtime timeline), spread over the steps
// they ride under the MFMAs.
struct DmaQ {
  const char* su;  // wave-uniform source of this wave's 6 KB share
  unsigned lds;    // LDS byte address of this wave's share
  bool on;
};
__device__ __forceinline__ void glds16c(const char* sbase, unsigned voff, unsigned lds_addr) {
  glds16((const float*)sbase, voff, lds_addr);
}
__device__ __forceinline__ void dmaq_issue(const DmaQ& j, int i, unsigned lane16) {
  if (j.on) glds16c(j.su + i * 1024, lane16, j.lds + i * 1024);
}
// Two consecutive 1 KB pieces in one statement: the immediate offset of global_load_lds advances
// BOTH the global source and the LDS destination (tools/dma_offset_probe.hip), so pieces that lie
// within 4 KB share one M0 setting and need no address arithmetic.  PAIR = 0, 1, 2 -> pieces
// (0,1), (2,3), (4,5) of the wave's 6 KB share.
template <int PAIR>
__device__ __forceinline__ void dmaq_issue2(const DmaQ& j, unsigned lane16) {
  if (!j.on) return;
  constexpr int BASE = (PAIR == 2) ? 4096 : 0;
  constexpr int O0 = (PAIR == 1) ? 2048 : 0, O1 = O0 + 1024;
  unsigned keep;
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2 offset:%4\n\t"
      "global_load_lds_dwordx4 %1, %2 offset:%5\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(lane16), "s"((const float*)(j.su + BASE)), "s"(j.lds + BASE), "n"(O0), "n"(O1)
      : "memory");
}

template <int TERMS, int PPW, typename Late>
__device__ __forceinline__ void gemm_q(f32x4 (&acc)[8], const u32x4 (&x)[3], lds_char* wq, unsigned lane16, const DmaQ& job, Late late) {
  if (TERMS == 1) {  // bf16 matrix mode: one term, leading pieces only
    u32x4 w1[2][2];
    lds_char* wl = wq + lane16;
#pragma unroll
    for (int q = 0; q < 2; ++q) w1[0][q] = *(lds_cu32x4*)(wl + q * 1024);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s + 1 < 4) {
#pragma unroll
        for (int q = 0; q < 2; ++q) w1[(s + 1) & 1][q] = *(lds_cu32x4*)(wl + (2 * (s + 1) + q) * 1024);
      }
      // one-term quarters are short (8 MFMAs): request the whole share of the quarter two ahead at step 0 instead of spread over
      // steps 0..2 -- half an iteration more lead on the L2 -> LDS latency (the drain's count only gets more conservative: hook
      // loads of steps 0..2 are now younger than the pieces and still counted as older).  configs[2] step 14.71-14.76 ->
      // 14.43-14.54 ms, alternating.  (PPW == 6, the backward chain: a pair of pieces per step, as in the six-term form.)
      if (PPW != 6) {
        if (s == 0) {
#pragma unroll
          for (int i = 0; i < PPW; ++i) dmaq_issue(job, i, lane16);
        }
      } else if (s < 3) {
        if (s == 0) dmaq_issue2<0>(job, lane16);
        else if (s == 1) dmaq_issue2<1>(job, lane16);
        else dmaq_issue2<2>(job, lane16);
      }
      late(s);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w1[s & 1][q], x[0], acc[2 * s + q]);
      __builtin_amdgcn_sched_barrier(0);
    }
    return;
  }
  // term order w3x1, w2x2, w2x1, w1x3, w1x2, w1x1 (roughly ascending magnitude): the w3 / w2
  // fragments are dead after one / three terms and are refilled in place for the next pair;
  // only w1 is double buffered.
  u32x4 w3[2], w2[2], w1[2][2];
  lds_char* wl = wq + lane16;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    w3[q] = *(lds_cu32x4*)(wl + 2 * 8192 + q * 1024);
    w2[q] = *(lds_cu32x4*)(wl + 1 * 8192 + q * 1024);
    w1[0][q] = *(lds_cu32x4*)(wl + q * 1024);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bool more = s + 1 < 4;
    const int nb = (2 * (s + 1)) * 1024;
    if (more) {
#pragma unroll
      for (int q = 0; q < 2; ++q) w1[(s + 1) & 1][q] = *(lds_cu32x4*)(wl + nb + q * 1024);
    }
    if (s < 3) {
      if (PPW == 6) {
        if (s == 0) dmaq_issue2<0>(job, lane16);
        else if (s == 1) dmaq_issue2<1>(job, lane16);
        else dmaq_issue2<2>(job, lane16);
      } else {
#pragma unroll
        for (int i = s * PPW / 3; i < (s + 1) * PPW / 3; ++i) dmaq_issue(job, i, lane16);
      }
    }
    late(s);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w3[q], x[0], acc[2 * s + q]);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int q = 0; q < 2; ++q) w3[q] = *(lds_cu32x4*)(wl + 2 * 8192 + nb + q * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w2[q], x[1], acc[2 * s + q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w2[q], x[0], acc[2 * s + q]);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int q = 0; q < 2; ++q) w2[q] = *(lds_cu32x4*)(wl + 1 * 8192 + nb + q * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w1[s & 1][q], x[2], acc[2 * s + q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w1[s & 1][q], x[1], acc[2 * s + q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(w1[s & 1][q], x[0], acc[2 * s + q]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

__device__ __forceinline__ bool x6_contig(const char* u0, const char* u1, const char* u2, const char* u3, const char* u4,
                                          const char* u5, const char* u6, const char* u7, int G) {
  const char* u[8] = {u0, u1, u2, u3, u4, u5, u6, u7};
  bool ok = true;
#pragma unroll
  for (int k = 1; k < 8; ++k) ok = ok && (k >= G || u[k] == u0 + (size_t)k * MGN_WPACK_BYTES);
  return ok;
}

template <typename T>
__device__ __forceinline__ T pick8(T a0, T a1, T a2, T a3, T a4, T a5, T a6, T a7, int i) {
  T lo = pick4(a0, a1, a2, a3, i);
  T hi = pick4(a4, a5, a6, a7, i - 4);
  return (i < 4) ? lo : hi;
}

// Wait until at most `n` (floored to a supported immediate) of the youngest VMEM operations are
// outstanding.  vmcnt retires in issue order: everything older than the n youngest has landed.
__device__ __forceinline__ void drain_allow(int n) {
  if (n >= 38)
    dma_drain_counted<38>();
  else if (n >= 30)
    dma_drain_counted<30>();
  else if (n >= 22)
    dma_drain_counted<22>();
  else if (n >= 14)
    dma_drain_counted<14>();
  else if (n >= 6)
    dma_drain_counted<6>();
  else
    dma_drain();
}

// The stream of quarters a persistent workgroup consumes: unit (q/4) % G, slice q % 4, ring slot
// q % 3.  The DMA runs TWO quarters ahead of the compute: the pieces issued in iteration q
// (quarter q+2) must have landed by the barrier that opens iteration q+2, i.e. they are drained
// at the end of iteration q+1, where every VMEM operation issued after them may stay in flight.
// `young` counts those operations -- only ones that are GUARANTEED to be issued (unconditional
// loads; stores of a wave that owns at least one valid row), so the count is a lower bound and
// the drain can only over-wait.
struct QStream {
  long issued;    // quarters whose DMA has been issued
  long total;     // quarters of the whole stream
  int du, dq;     // unit / slice of the next quarter to issue
  int dslot;      // ring slot of the next quarter to issue
  int cslot;      // ring slot of the next quarter to compute
  int young;      // VMEM operations issued since the DMA pieces of the previous iteration
};

// ---- Loads the compiler does NOT track (static-shape instantiations only).
// hipcc cannot count the VMEM operations between a load and its use across the rolled unit loop, and it does not
// see the DMA pieces at all, so every compiler-tracked load that is consumed in a later unit costs an
// `s_waitcnt vmcnt(0)` at its use: a wait for EVERYTHING in flight -- the weight quarters just requested from L2
// and the row stores just issued (six per tile in the edge update: 35 % of the wave's cycles sit in
// SQ_WAIT_INST_ANY, profiles/r02_pmc_stall_counters.csv).  In the instantiations whose unit structure is a
// compile-time constant (ShEdge / ShNode below: the unit loop unrolls, every load is an unconditional statement
// of one straight-line tile body) operand rows and row indices are fetched by inline asm and ordered by the SAME
// counted drains as the DMA: vmcnt retires in issue order and the drain that closes quarter q+1 waits for the
// DMA pieces of quarter q, so a load issued in quarter q before that quarter's last piece (steps 0..2) has
// landed when quarter q+1 ends, a load of step 3 when quarter q+2 ends.  Every use is at least that far away,
// and tools/check_untracked_loads.py asserts on the ISA that nothing touches a destination register in between
// (the asm result is a fresh value of straight-line code: no phi, hence no copy, until the tile loop's latch).
template <int S>
__device__ __forceinline__ void ld2u_at(f32x4& d0, f32x4& d1, const float* rowp) {
  asm volatile("global_load_dwordx4 %0, %2, off offset:%3\n\t"
               "global_load_dwordx4 %1, %2, off offset:%4"
               : "=&v"(d0), "=&v"(d1)
               : "v"(rowp), "n"(128 * S), "n"(128 * S + 64)
               : "memory");
}
// blocks 2s, 2s+1 of a T-layout row tile (rowp = row base + 4g); s is a constant after unrolling
__device__ __forceinline__ void ld2u(f32x4 (&dst)[8], const float* rowp, int s, int& n) {
  if (s == 0) ld2u_at<0>(dst[0], dst[1], rowp);
  else if (s == 1) ld2u_at<1>(dst[2], dst[3], rowp);
  else if (s == 2) ld2u_at<2>(dst[4], dst[5], rowp);
  else ld2u_at<3>(dst[6], dst[7], rowp);
  n += 2;
}
// a whole row tile in the first THREE steps of a quarter (3 + 3 + 2 blocks): all of it is older than the quarter's
// last DMA piece, i.e. has landed when the NEXT quarter ends
template <int B0, int NB>
__device__ __forceinline__ void ldnu_at(f32x4& d0, f32x4& d1, f32x4& d2, const float* rowp) {
  if (NB == 3)
    asm volatile("global_load_dwordx4 %0, %3, off offset:%4\n\t"
                 "global_load_dwordx4 %1, %3, off offset:%5\n\t"
                 "global_load_dwordx4 %2, %3, off offset:%6"
                 : "=&v"(d0), "=&v"(d1), "=&v"(d2)
                 : "v"(rowp), "n"(64 * B0), "n"(64 * B0 + 64), "n"(64 * B0 + 128)
                 : "memory");
  else
    asm volatile("global_load_dwordx4 %0, %2, off offset:%3\n\t"
                 "global_load_dwordx4 %1, %2, off offset:%4"
                 : "=&v"(d0), "=&v"(d1)
                 : "v"(rowp), "n"(64 * B0), "n"(64 * B0 + 64)
                 : "memory");
}
__device__ __forceinline__ void ld3u(f32x4 (&dst)[8], const float* rowp, int s, int& n) {
  if (s == 0) {
    ldnu_at<0, 3>(dst[0], dst[1], dst[2], rowp);
    n += 3;
  } else if (s == 1) {
    ldnu_at<3, 3>(dst[3], dst[4], dst[5], rowp);
    n += 3;
  } else if (s == 2) {
    ldnu_at<6, 2>(dst[6], dst[7], dst[7], rowp);
    n += 2;
  }
}
__device__ __forceinline__ int ldiu(const int32_t* p) {
  int v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// Use-site fence of an untracked index: what is computed from it is emitted after this point (a volatile asm is
// neither hoisted nor speculated), i.e. after the drains that ordered the load.  Emits no code.
__device__ __forceinline__ int landed(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ---- Shape policies of k_mlp_fwd_x6.  ShDyn: everything read from the arguments (any launch the packed path
// accepts; rolled unit loop, compiler-tracked loads).  Static shapes: the two launches a message-passing round
// spends its time in; chosen by launch_fwd only when the arguments match field by field.
struct ShDyn {
  static constexpr bool ST = false;
  static __device__ __forceinline__ int nphase(const mgn_mlp_fwd_args& a) { return a.nphase; }
  static __device__ __forceinline__ int NL(const mgn_mlp_fwd_args& a) { return a.NL; }
  static __device__ __forceinline__ int n_add(const mgn_mlp_fwd_args& a) { return a.n_add; }
  static __device__ __forceinline__ int n_post(const mgn_mlp_fwd_args& a) { return a.n_post; }
  static __device__ __forceinline__ bool resid(const mgn_mlp_fwd_args& a) { return a.resid != nullptr; }
  static __device__ __forceinline__ bool scale(const mgn_mlp_fwd_args& a) { return a.scale != nullptr; }
  static __device__ __forceinline__ bool seg(const mgn_mlp_fwd_args& a) { return a.seg_out != nullptr; }
  static __device__ __forceinline__ bool has_idx(const int32_t* p) { return p != nullptr; }
  static __device__ __forceinline__ bool has_addidx(const int32_t* p) { return p != nullptr; }
};
// edge update of a round: e' = e + RMSNorm(MLP(W_e e + Pd[dst] + Ps[src])), aggregation by dst fused
// (rows contiguous, both projections gathered through index rows, seg_key == add_idx[0])
struct ShEdge {
  static constexpr bool ST = true;
  static __device__ __forceinline__ constexpr int nphase(const mgn_mlp_fwd_args&) { return 1; }
  static __device__ __forceinline__ constexpr int NL(const mgn_mlp_fwd_args&) { return 4; }
  static __device__ __forceinline__ constexpr int n_add(const mgn_mlp_fwd_args&) { return 2; }
  static __device__ __forceinline__ constexpr int n_post(const mgn_mlp_fwd_args&) { return 0; }
  static __device__ __forceinline__ constexpr bool resid(const mgn_mlp_fwd_args&) { return true; }
  static __device__ __forceinline__ constexpr bool scale(const mgn_mlp_fwd_args&) { return true; }
  static __device__ __forceinline__ constexpr bool seg(const mgn_mlp_fwd_args&) { return true; }
  static __device__ __forceinline__ constexpr bool has_idx(const int32_t*) { return false; }
  static __device__ __forceinline__ constexpr bool has_addidx(const int32_t*) { return true; }
};
// node update of a round: x' = x + RMSNorm(MLP([x, agg])), NPOST post-products (the next round's projections)
template <int NPOST>
struct ShNode {
  static constexpr bool ST = true;
  static __device__ __forceinline__ constexpr int nphase(const mgn_mlp_fwd_args&) { return 2; }
  static __device__ __forceinline__ constexpr int NL(const mgn_mlp_fwd_args&) { return 4; }
  static __device__ __forceinline__ constexpr int n_add(const mgn_mlp_fwd_args&) { return 0; }
  static __device__ __forceinline__ constexpr int n_post(const mgn_mlp_fwd_args&) { return NPOST; }
  static __device__ __forceinline__ constexpr bool resid(const mgn_mlp_fwd_args&) { return true; }
  static __device__ __forceinline__ constexpr bool scale(const mgn_mlp_fwd_args&) { return true; }
  static __device__ __forceinline__ constexpr bool seg(const mgn_mlp_fwd_args&) { return false; }
  static __device__ __forceinline__ constexpr bool has_idx(const int32_t*) { return false; }
  static __device__ __forceinline__ constexpr bool has_addidx(const int32_t*) { return false; }
};

// blocks 2s, 2s+1 of a T-layout row tile (rowp = row base + 4g): two of the 8 loads of a tile
__device__ __forceinline__ void ld2(f32x4 (&dst)[8], const float* rowp, int s, int& n) {
  dst[2 * s] = ld4(rowp + 32 * s);
  dst[2 * s + 1] = ld4(rowp + 32 * s + 16);
  n += 2;
}

// Walk of the row tiles by a persistent workgroup: tile b, b + gridDim, ... (neighbouring tiles run at the same
// time on neighbouring workgroups = on all 8 XCDs).  An XCD-aware walk (a contiguous eighth of the tiles per XCD)
// was measured 1 % slower: DESIGN.md section 9.
struct TileWalk {
  long first, end, stride;  // this workgroup's tiles: first, first + stride, ... < end
  long count;
};
__device__ __forceinline__ TileWalk tile_walk(long ntiles) {
  TileWalk w;
  const unsigned G = gridDim.x, b = blockIdx.x;
  w.first = b, w.end = ntiles, w.stride = G;
  w.count = (w.first < w.end) ? (w.end - w.first + w.stride - 1) / w.stride : 0;
  return w;
}

// Segmented sum over the 16 rows of a wave tile (rows sorted by `key`, T-layout values v[ib]): a segmented
// inclusive scan over the 16 lanes of a DPP row leaves every run's sum in its last lane; a run that lies
// inside the tile is a finished segment -> seg_out[key]; a run cut by the tile boundary goes to
// seg_part[wave tile][0 = began before | 1 = continues after] for mgn_seg_fix.  Clobbers v.
// PRE: instead of reading the run's bounds from seg_rowptr (two dependent loads per run end in the epilogue's
// critical path), the caller passes the keys of the rows just before and just after the wave tile (kprev / knext2:
// wave-uniform, -1 outside the row range): a run began before the tile iff it contains the tile's first row and
// that row has the previous row's key; it continues after the tile iff it ends in lane 15 and the next row has its key.
// The scan itself: after it lane c of every DPP row holds the sum of v over the run of equal keys that ends at row c.
__device__ __forceinline__ void seg_scan16(f32x4 (&v)[8], int key) {
  constexpr int HB = 8;
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    int kd;
    if (st == 0) kd = __builtin_amdgcn_update_dpp(-2, key, 0x111, 0xf, 0xf, false);
    else if (st == 1) kd = __builtin_amdgcn_update_dpp(-2, key, 0x112, 0xf, 0xf, false);
    else if (st == 2) kd = __builtin_amdgcn_update_dpp(-2, key, 0x114, 0xf, 0xf, false);
    else kd = __builtin_amdgcn_update_dpp(-2, key, 0x118, 0xf, 0xf, false);
    const float same = (kd == key) ? 1.f : 0.f;
    // One instruction per value and step: v_fmac with a DPP-shifted first operand,
    //   v[c] += v[c - d] * same[c]      (lanes c < d read 0: bound_ctrl)
    // in inline asm -- with __builtin_amdgcn_update_dpp on the 32 accumulator elements hipcc
    // (ROCm 7.2) re-used the shifted copy of one element for another.  The s_nop 1 covers the
    // 2 wait states a DPP read needs after a VALU write of its source (the sources were
    // written a whole step -- 32 instructions -- earlier; the nop guards the block's first).
#define X6_FMAC_DPP4(N)                                                                                   \
  asm volatile("s_nop 1\n\t"                                                                               \
               "v_fmac_f32_dpp %0, %0, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"      \
               "v_fmac_f32_dpp %1, %1, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"      \
               "v_fmac_f32_dpp %2, %2, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"      \
               "v_fmac_f32_dpp %3, %3, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1"            \
               : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3)                                                     \
               : "v"(same))
#pragma unroll
    for (int ib = 0; ib < HB; ++ib) {
      float v0 = v[ib][0], v1 = v[ib][1], v2 = v[ib][2], v3 = v[ib][3];
      if (st == 0) X6_FMAC_DPP4(1);
      else if (st == 1) X6_FMAC_DPP4(2);
      else if (st == 2) X6_FMAC_DPP4(4);
      else X6_FMAC_DPP4(8);
      v[ib][0] = v0, v[ib][1] = v1, v[ib][2] = v2, v[ib][3] = v3;
    }
#undef X6_FMAC_DPP4
  }
}
template <bool PRE = false>
__device__ __forceinline__ void seg_scan_store(f32x4 (&v)[8], int key, long wtile, const int32_t* __restrict__ seg_rowptr,
                                               float* __restrict__ seg_out, float* __restrict__ seg_part, int g,
                                               int kprev = -1, int knext2 = -1) {
  constexpr int HB = 8, H = 128;
  seg_scan16(v, key);
  const int knext = __builtin_amdgcn_update_dpp(-3, key, 0x101, 0xf, 0xf, false);  // row_shl:1, lane 15 keeps -3
  const int key0 = __builtin_amdgcn_readfirstlane(key);  // key of the tile's first row (all lanes active here)
  if (key >= 0 && knext != key) {  // run end
    const long r0 = wtile * 16;
    bool before, inside;
    if (PRE) {
      before = (key == key0) && (kprev == key0);
      inside = !before && !(knext == -3 && knext2 == key);  // knext == -3: the run ends in lane 15
    } else {
      const int beg = seg_rowptr[key], end = seg_rowptr[key + 1];
      before = beg < r0;
      inside = beg >= r0 && end <= r0 + 16;
    }
    float* dst;
    if (inside)
      dst = seg_out + (long)key * H;
    else
      dst = seg_part + (wtile * 2 + (before ? 0 : 1)) * H;
#pragma unroll
    for (int ib = 0; ib < HB; ++ib) st4(dst + 4 * g + 16 * ib, v[ib]);
  }
}

// ------------------------------------------------------------------------ forward
// Same contract as k_mlp_fwd_lds (persistent workgroups, 64-row tiles, 16 rows per wave); the
// GEMM units come packed in a.wpk[u], u in stream order: phases of layer 0, layers 1..NL-1,
// post-products.
// NW waves per workgroup: 4 (two workgroups per CU, ring of 3 quarters, DMA two ahead) or 8 (one
// workgroup per CU: the weight stream is shared by twice the rows -- half the DMA issues and
// L2->LDS bytes per row -- and the ring holds 6 quarters, DMA five ahead), or 6 (MGN_NW=6, experiment: two workgroups per CU =
// THREE waves per SIMD at <= 168 VGPRs, the occupancy lever of VERDICT r2 item 3; 96-row tiles, ring of 3 quarters).
template <int TERMS, int NW, int ACT, class SH = ShDyn>
__global__ void __launch_bounds__(64 * NW, (NW == 6 ? 3 : 2)) k_mlp_fwd_x6(const mgn_mlp_fwd_args a) {
  // unit structure: constants in the static shapes (the unit loop unrolls, loads go untracked), arguments in ShDyn
  const int NPH = SH::nphase(a), NLL = SH::NL(a), NADD = SH::n_add(a), NPOST = SH::n_post(a);
  const bool HAS_RESID = SH::resid(a), HAS_SCALE = SH::scale(a), HAS_SEG = SH::seg(a);
  constexpr bool UT = SH::ST;
  // the three-wave instance spills: an index the compiler parks in scratch right after its load must be a load it tracks
  // (tools/check_untracked_loads.py found exactly that); the row loads stay untracked
  constexpr bool UI = UT && NW != 6;
  constexpr int RING = (NW == 8) ? 6 : 3;
  constexpr int AHEAD = RING - 1;
  // 1 KB DMA pieces per wave and quarter.  [r4] bf16 matrix mode (TERMS == 1) multiplies by the LEADING bf16 piece only -- the first
  // 8 KB of a packed quarter -- so only that third travels L2 -> LDS (the weight stream was 1.8x the row traffic of a tile in pieces)
  constexpr int PPW = (TERMS == 1) ? 8 / NW : 24 / NW;
  static_assert(24 % NW == 0 && (TERMS != 1 || 8 % NW == 0), "the quarter is shared out in whole 1 KB pieces");
  constexpr int WSHARE = PPW * 1024;
  constexpr int HB = 8, H = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* ring = (lds_char*)smem;
  lds_char* cst = ring + RING * X6_QBYTES;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const unsigned lane16 = 16u * lane;
  TL_DECL();
  const long ntiles = (a.M + 16 * NW - 1) / (16 * NW);
  const TileWalk tw = tile_walk(ntiles);
  long tile = tw.first;
  if (tw.count == 0) return;
  const long my_tiles = tw.count;
  const int GL = NPH + NLL - 1;
  const int G = GL + NPOST;
  const char *U0 = (const char*)a.wpk[0], *U1 = (const char*)a.wpk[1], *U2 = (const char*)a.wpk[2], *U3 = (const char*)a.wpk[3];
  const char *U4 = (const char*)a.wpk[4], *U5 = (const char*)a.wpk[5], *U6 = (const char*)a.wpk[6], *U7 = (const char*)a.wpk[7];
  // packed units laid out back to back (the usual case): one multiply instead of a select chain per quarter
  const bool contig = x6_contig(U0, U1, U2, U3, U4, U5, U6, U7, G);
  float *sH0 = a.saveH[0], *sH1 = a.saveH[1], *sH2 = a.saveH[2];
  uint32_t *sM0 = a.saveM[0], *sM1 = a.saveM[1], *sM2 = a.saveM[2];
  float *sZ0 = a.saveZ[0], *sZ1 = a.saveZ[1], *sZ2 = a.saveZ[2];
  const float *src0 = a.src[0], *src1 = a.src[1], *src2 = a.src[2];
  const int32_t *idx0 = a.idx[0], *idx1 = a.idx[1], *idx2 = a.idx[2];
  const float *as0 = a.add_src[0], *as1 = a.add_src[1];
  const int32_t *ai0 = a.add_idx[0], *ai1 = a.add_idx[1];
  const unsigned ring0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring));
  // index loads one rows_of() issues (all unconditional)
  const bool I0 = SH::has_idx(idx0), I1 = NPH > 1 && SH::has_idx(idx1), I2 = NPH > 2 && SH::has_idx(idx2);
  const bool A0 = NADD > 0 && SH::has_addidx(ai0), A1 = NADD > 1 && SH::has_addidx(ai1);
  const int n_idx = (I0 ? 1 : 0) + (I1 ? 1 : 0) + (I2 ? 1 : 0) + (A0 ? 1 : 0) + (A1 ? 1 : 0);

  QStream qs;
  qs.issued = 0, qs.total = my_tiles * 4 * G, qs.du = 0, qs.dq = 0, qs.dslot = 0, qs.cslot = 0, qs.young = 0;
  auto next_job = [&]() -> DmaQ {
    DmaQ j;
    const char* up = contig ? U0 + (size_t)qs.du * MGN_WPACK_BYTES : pick8(U0, U1, U2, U3, U4, U5, U6, U7, qs.du);
    j.su = (const char*)uniform_ptr((const float*)(up + qs.dq * X6_QBYTES + wv * WSHARE));
    j.lds = ring0 + qs.dslot * X6_QBYTES + wv * WSHARE;
    j.on = qs.issued < qs.total;
    ++qs.issued;
    qs.dslot = (qs.dslot == RING - 1) ? 0 : qs.dslot + 1;
    if (++qs.dq == 4) {
      qs.dq = 0;
      qs.du = (qs.du + 1 == G) ? 0 : qs.du + 1;
    }
    return j;
  };
  // prologue: the first AHEAD quarters in flight
#pragma unroll
  for (int k = 0; k < AHEAD; ++k) {
    const DmaQ j0 = next_job();
#pragma unroll
    for (int i = 0; i < PPW; ++i) dmaq_issue(j0, i, lane16);
  }
  for (int i = threadIdx.x; i < 5 * H; i += 64 * NW) {
    const int l = i >> 7, jx = i & 127;
    const float* bp = (l == 4) ? a.scale : pick4(a.b[0], a.b[1], a.b[2], a.b[3], l);
    ((__attribute__((address_space(3))) float*)cst)[i] = (bp != nullptr && (l == 4 || l < NLL)) ? bp[jx] : 0.f;
  }
  auto lds_bias = [&](f32x4 (&acc)[HB], int l) {
#pragma unroll
    for (int ib = 0; ib < HB; ++ib) acc[ib] = *(lds_cf32x4*)(cst + l * 512 + 64 * ib + 16 * g);
  };
  // U: index loads untracked (the next tile's, issued under unit 0; first use a unit later)
  auto rows_of = [&](long tl, long& mm, bool& valid, int (&rid)[5], auto U) {
    constexpr bool UL = decltype(U)::value;
    const long m = (tl * NW + wv) * 16 + c;
    valid = m < a.M;
    mm = valid ? m : a.M - 1;  // waves past M still take part in the DMA / barriers
    auto ldx = [&](const int32_t* ip) -> int {
      if constexpr (UL) return ldiu(ip + mm);
      else return ip[mm];
    };
    rid[0] = I0 ? ldx(idx0) : (int)mm;
    rid[1] = (NPH > 1) ? (I1 ? ldx(idx1) : (int)mm) : 0;
    rid[2] = (NPH > 2) ? (I2 ? ldx(idx2) : (int)mm) : 0;
    rid[3] = (NADD > 0) ? (A0 ? ldx(ai0) : (int)mm) : 0;
    rid[4] = (NADD > 1) ? (A1 ? ldx(ai1) : (int)mm) : 0;
  };
  // row loads of the `late` hooks: untracked in the static shapes
  auto LD2 = [&](f32x4 (&dst)[8], const float* rowp, int s, int& n) {
    if constexpr (UT) ld2u(dst, rowp, s, n);
    else ld2(dst, rowp, s, n);
  };
  auto LANDED = [&](int v) -> int {
    if constexpr (UT) return landed(v);
    else return v;
  };
  long mm;
  bool valid;
  int rid[5];
  // static shapes with a fused segment sum: the row's key is its first gather index (seg_key == add_idx[0],
  // checked by launch_fwd) and the keys of the rows either side of the wave tile come in ONE late load
  // (lanes c < 8: row r0 - 1, lanes c >= 8: row r0 + 16)
  int nbk = 0;
  rows_of(tile, mm, valid, rid, std::false_type{});
  // Registers are shared by hand (the unit loop is rolled, so the compiler sees every array live
  // across it): `pr` = first gathered projection, later the residual rows; `nin` = rows of the
  // next phase / tile, and the second gathered projection in between (n_add needs nphase == 1,
  // and NL >= 2 when there is a residual -- checked on the host).
  f32x4 nin[HB], acc[HB], pr[HB];
  u32x4 xs[4][3];
#pragma unroll
  for (int kb = 0; kb < HB; ++kb) nin[kb] = ld4(src0 + (long)rid[0] * H + 4 * g + 16 * kb);
  dma_drain();
  __syncthreads();

  // one GEMM unit = 4 quarters of the stream; `late` = the unit's operand prefetch (first quarter)
  auto run_unit = [&](auto late) {
#pragma unroll
    for (int jq = 0; jq < 4; ++jq) {
      TL_STAMP(3);
      __syncthreads();  // quarter landed everywhere; the slot of two quarters ago is free again
      TL_STAMP(4);
      const DmaQ job = next_job();
      const int before = qs.young;
      qs.young = 0;
      int early = 0;  // loads of steps 0..2: older than this quarter's last DMA piece
      gemm_q<TERMS, PPW>(acc, xs[jq], ring + qs.cslot * X6_QBYTES, lane16, job, [&](int s) { late(jq, s, (s < 3) ? early : qs.young); });
      qs.cslot = (qs.cslot == RING - 1) ? 0 : qs.cslot + 1;
      TL_STAMP(5);
      if (AHEAD == 2) {
        drain_allow(before + (job.on ? PPW : 0) + early + qs.young);
      } else {
        // the quarter computed next was issued AHEAD-1 iterations ago; at least PPW*(AHEAD-1)
        // operations (the pieces of the iterations since) are younger -- if they were all issued
        if (job.on)
          dma_drain_counted<PPW*(AHEAD - 1)>();
        else
          dma_drain();
      }
      TL_STAMP(6);
    }
  };

  for (; tile < tw.end; tile += tw.stride) {
    const long ntile = tile + tw.stride;
    const bool has_next = ntile < tw.end;
    const bool wvalid = __builtin_amdgcn_readfirstlane((int)((tile * NW + wv) * 16 < a.M));  // stores below do issue
    long mmn;
    bool validn;
    int ridn[5];
    TL_STAMP(1);
#pragma unroll
    for (int p = 0; p < 5; ++p) rid[p] = LANDED(rid[p]);
    lds_bias(acc, 0);
    auto unit_body = [&](int u) {
      if (u < NPH) {
        // (NW == 6, 168 registers: the selector of the matrix-pipe split pushed freshly loaded rows into scratch -- tests/test_untracked_loads_isa.py)
        split_tile<TERMS, NW != 6>(nin, xs);  // rows of phase u (loaded under the previous unit / tile)
      } else {  // layer l >= 1: operand = ReLU(previous accumulator)
        const int l = u - NPH + 1;
        if (l == 1) {
          if (NADD > 0) {
#pragma unroll
            for (int ib = 0; ib < HB; ++ib) acc[ib] += pr[ib];
          }
          if (NADD > 1) {
#pragma unroll
            for (int ib = 0; ib < HB; ++ib) acc[ib] += nin[ib];
          }
        }
        if (ACT == MGN_ACT_SILU) {  // pre-activations first (the backward's silu'), then h = z * sigmoid(z)
          float* sz = pick3(sZ0, sZ1, sZ2, l - 1);
          if (sz != nullptr) {
            if (valid) {
#pragma unroll
              for (int ib = 0; ib < HB; ++ib) st4_stream(sz + mm * H + 4 * g + 16 * ib, acc[ib]);
            }
            if (wvalid) qs.young += 8;
          }
#pragma unroll
          for (int ib = 0; ib < HB; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ib][r] = silu_f(acc[ib][r]);
        } else {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float v = acc[ib][r];
              asm("v_max_f32 %0, 0, %0" : "+v"(v));  // one instruction (fmaxf also quiets NaNs: two)
              acc[ib][r] = v;
            }
        }
        float* sh = pick3(sH0, sH1, sH2, l - 1);
        // [r4] precision == 2 (bf16 matrix mode with two-byte saves): the saved activation IS the bf16 operand of the next layer, so the
        // row is stored as the four packed leading pieces of the split below (256 bytes: K-slice p at bf16 offset 32 p, lane g's 16
        // bytes = features 32p + 4g .. + 3 and 32p + 16 + 4g .. + 3) -- what k_wgrad_x6<1> reads back (negative ldb)
        const bool s16 = (TERMS == 1) && a.precision == 2;
        if (sh != nullptr && !s16) {
          if (valid) {
#pragma unroll
            for (int ib = 0; ib < HB; ++ib) st4_stream(sh + mm * H + 4 * g + 16 * ib, acc[ib]);
          }
          if (wvalid) qs.young += 8;
        }
        uint32_t* smk = (ACT == MGN_ACT_SILU) ? nullptr : pick3(sM0, sM1, sM2, l - 1);
        if (smk != nullptr) {  // ReLU mask as bits: all the backward chain needs of this activation
          u32 bits = 0;
#pragma unroll
          for (int ib = 0; ib < HB; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // ReLU output: > 0 iff its integer image is > 0; med3(x, 0, 1) | shift-or: 2 instructions per value
              const float hval = acc[ib][r];  // (a scalar copy first: __builtin_bit_cast of a vector ELEMENT read element 0 for all four)
              int t = __builtin_bit_cast(int, hval);
              t = (t < 0) ? 0 : ((t > 1) ? 1 : t);  // v_med3_i32
              bits |= (u32)t << (4 * ib + r);      // v_lshl_or_b32
            }
          if (valid) *(__attribute__((address_space(1))) u32*)(smk + mm * 4 + g) = bits;
          if (wvalid) qs.young += 1;
        }
        split_tile<TERMS, NW != 6>(acc, xs);
        if (TERMS == 1 && sh != nullptr && s16) {
          if (valid) {
#pragma unroll
            for (int pq = 0; pq < 4; ++pq)
              st4_stream((float*)((char*)sh + (size_t)(mm * H + 32 * pq + 8 * g) * 2), __builtin_bit_cast(f32x4, xs[pq][0]));
          }
          if (wvalid) qs.young += 4;
        }
        lds_bias(acc, l);
      }
      run_unit([&](int jq, int s, int& n) {
        if (jq == 0) {
          if (u == 0 && s == 0) {  // the next tile's row indices (first use: a unit later)
            rows_of(has_next ? ntile : tile, mmn, validn, ridn, std::integral_constant<bool, UI>{});
            n += n_idx;
          }
          if (u == 0 && NADD > 0)  // first gathered projection (used after this unit)
            LD2(pr, as0 + (long)rid[3] * H + 4 * g, s, n);
          else if (u == GL - 1 && NLL > 1 && HAS_RESID)  // residual rows (used in the epilogue)
            LD2(pr, a.resid + mm * H + 4 * g, s, n);
        } else if (jq == 1) {
          if (u < NPH) {
            if (u + 1 < NPH)  // rows of the next phase (split once this unit's last drain has passed)
              LD2(nin, pick3(src0, src1, src2, u + 1) + (long)((u == 0) ? rid[1] : rid[2]) * H + 4 * g, s, n);
            else if (NADD > 1)  // second gathered projection
              LD2(nin, as1 + (long)rid[4] * H + 4 * g, s, n);
          }
          // the next tile's rows (static shapes: unconditionally -- the last tile re-reads its own rows, which
          // keeps the load an unconditional statement)
          if (u == GL - 1 && NLL > 1 && NPOST == 0 && (UT || has_next))
            LD2(nin, src0 + (long)LANDED(ridn[0]) * H + 4 * g, s, n);
        } else if (jq == 2) {
          if (UT && HAS_SEG && u == GL - 1 && s == 0) {  // keys of the rows either side of the wave tile
            const long r0 = (tile * NW + wv) * 16;
            const long rk = (c < 8) ? ((r0 > 0) ? r0 - 1 : 0) : ((r0 + 16 < a.M) ? r0 + 16 : a.M - 1);
            if constexpr (UI) nbk = ldiu(a.seg_key + rk);
            else if constexpr (UT) nbk = a.seg_key[rk];
            n += 1;
          }
        }
      });
    };
    if constexpr (UT) {
#pragma unroll
      for (int u = 0; u < SH::nphase(a) + SH::NL(a) - 1; ++u) unit_body(u);
    } else {
      for (int u = 0; u < GL; ++u) unit_body(u);
    }
    if (NLL == 1) {  // no layer 1 to add the gathered projections at; operands fetched late
      if (NADD > 0) {
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) acc[ib] += pr[ib];
      }
      if (NADD > 1) {
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) acc[ib] += nin[ib];
      }
      if (HAS_RESID) {
#pragma unroll
        for (int kb = 0; kb < HB; ++kb) pr[kb] = ld4(a.resid + mm * H + 4 * g + 16 * kb);
      }
      if (NPOST == 0 && has_next) {
        const long rn = LANDED(ridn[0]);
#pragma unroll
        for (int kb = 0; kb < HB; ++kb) nin[kb] = ld4(src0 + rn * H + 4 * g + 16 * kb);
      }
    }
    // ---- epilogue: RMSNorm (reference epsilon placement), residual, stores
    TL_STAMP(7);
    {
      float inv = 1.f;
      if (HAS_SCALE) {
        float ss = 0.f;
#pragma unroll
        for (int ib = 0; ib < HB; ++ib)
#pragma unroll
          for (int r = 0; r < 4; ++r) ss = fmaf(acc[ib][r], acc[ib][r], ss);
        ss = rowsum4(ss);
        const float rms = sqrtf(ss) / sqrtf((float)H);
        inv = 1.0f / (rms + a.eps);
        if (a.saveR != nullptr && valid && g == 0) st1(a.saveR + mm, rms);
      }
      const long ro = mm * H + 4 * g;
#pragma unroll
      for (int ib = 0; ib < HB; ++ib) {
        f32x4 y = acc[ib];
        if (HAS_SCALE) {
          const f32x4 u = y * inv;
          if (a.saveU != nullptr && valid) st4_stream(a.saveU + ro + 16 * ib, u);
          y = *(lds_cf32x4*)(cst + 4 * 512 + 64 * ib + 16 * g) * u;
        }
        if (a.y_out != nullptr && valid) st4(a.y_out + ro + 16 * ib, y);
        f32x4 yo = y;
        if (HAS_RESID) yo = pr[ib] + y;
        if (valid) st4(a.out + ro + 16 * ib, yo);
        acc[ib] = HAS_SEG ? y : yo;  // segment sum of the un-residualed y (the message)
      }
      if (wvalid) qs.young += 8 + ((HAS_SCALE && a.saveU != nullptr) ? 8 : 0) + ((a.y_out != nullptr) ? 8 : 0);
    }
    TL_STAMP(9);
    // ---- fused segment sum of y over runs of equal seg_key (rows are key-sorted): the aggregation
    //      of the edge messages without writing them.  Segmented inclusive scan over the 16 rows
    //      of the wave tile (lanes c of one DPP row), then the run ends store: a run that lies
    //      inside the tile is a finished segment -> seg_out[key]; a run cut by the tile boundary
    //      goes to seg_part[wave tile][0 = began before | 1 = continues after] for mgn_seg_fix.
    if (HAS_SEG) {
      if constexpr (UT) {
        const long r0 = (tile * NW + wv) * 16;
        const int nb = landed(nbk);
        const int kprev = (r0 > 0) ? __builtin_amdgcn_readlane(nb, 0) : -1;
        const int knxt = (r0 + 16 < a.M) ? __builtin_amdgcn_readlane(nb, 15) : -1;
        TL_STAMP(10);
        seg_scan_store<true>(acc, valid ? rid[3] : -1, (tile * NW + wv), a.seg_rowptr, a.seg_out, a.seg_part, g, kprev, knxt);
      } else {
        seg_scan_store(acc, valid ? a.seg_key[mm] : -1, (tile * NW + wv), a.seg_rowptr, a.seg_out, a.seg_part, g);
      }
    }
    // ---- post-products of the fresh output rows (next round's node projections)
    if (NPOST > 0) {
      split_tile<TERMS, NW != 6>(acc, xs);
      auto post_body = [&](int q) {
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) acc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        run_unit([&](int jq, int s, int& n) {
          if (jq == 0 && q == NPOST - 1 && (UT || has_next)) LD2(nin, src0 + (long)LANDED(ridn[0]) * H + 4 * g, s, n);
        });
        float* po = (q == 0) ? a.post_out[0] : a.post_out[1];
        if (valid) {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib) st4(po + mm * H + 4 * g + 16 * ib, acc[ib]);
        }
        if (wvalid) qs.young += 8;
      };
      if constexpr (UT) {
#pragma unroll
        for (int q = 0; q < SH::n_post(a); ++q) post_body(q);
      } else {
        for (int q = 0; q < NPOST; ++q) post_body(q);
      }
    }
    mm = mmn;
    valid = validn;
#pragma unroll
    for (int p = 0; p < 5; ++p) rid[p] = ridn[p];
    TL_STAMP(8);
  }
  TL_DUMP();
}

// ----------------------------------------------------------------------- backward
// Same contract as k_mlp_bwd_lds (persistent, 64-row tiles); GEMM units packed in a.wpk[u] in
// stream order: WT[NL-1], ..., WT[1], then WT0[0] when n_din == 1.  The gradient rows are split
// into bf16x3 exactly like forward activations (bf16 keeps the fp32 exponent range, so small
// gradients need no loss scaling).
// LDS: [ring of 3 quarters][scale 512 B][4 waves x NUSED column-sum slots x 512 B].  Only the REQUESTED
// column sums get a slot (the processor asks for dscale alone: bias gradients are a by-product of the
// weight-gradient kernel) -- with all NL + 1 slots the workgroup needed 84 480 B and only ONE fitted
// into the CU's 160 KB; with one slot it is 76 288 B like the forward kernel: two per CU.
#define X6_BWD_LDS_BYTES(NUSED) (X6_RING * X6_QBYTES + 512 + 4 * (NUSED) * 128 * 4)
// One step of the halving butterfly over the 16 rows of a wave tile (dscale, below): a lane keeps one half of its
// values and hands the other half to lane c ^ (1 << ST).  A template so that both trip counts are constants of
// the FIRST unrolling pass: with `n = 16 >> st` of an enclosing loop, the fully unrolled static-shape body left
// v[] indexed by a select of indices (compare chains and 76 spilled registers).
template <int ST>
__device__ __forceinline__ void fold_step(float (&v)[32], int c) {
  constexpr int n = 16 >> ST;  // values kept after this step
  const bool up = (c >> ST) & 1;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    const float lo = v[i], hi = v[i + n];
    const float keep = up ? hi : lo;
    const float send = up ? lo : hi;
    v[i] = keep + __shfl_xor(send, 1 << ST);
  }
}
// Shape policies (see ShDyn / ShEdge of the forward kernel).  SbEdge = the edge chain of a round: 4 layers, one
// input-gradient unit with a residual, RMSNorm, the second gradient stream (dOut2 = the aggregate's gradient)
// gathered through idx2, ReLU masks as bit words; no front stage, no fused segment sum.
struct SbDyn {
  static constexpr bool ST = false;
  static __device__ __forceinline__ int NL(const mgn_mlp_bwd_args& a) { return a.NL; }
  static __device__ __forceinline__ int n_din(const mgn_mlp_bwd_args& a) { return a.n_din; }
  static __device__ __forceinline__ bool scale(const mgn_mlp_bwd_args& a) { return a.scale != nullptr; }
  static __device__ __forceinline__ bool din_resid(const mgn_mlp_bwd_args& a) { return a.din_resid[0] != nullptr; }
};
struct SbEdge {
  static constexpr bool ST = true;
  static __device__ __forceinline__ constexpr int NL(const mgn_mlp_bwd_args&) { return 4; }
  static __device__ __forceinline__ constexpr int n_din(const mgn_mlp_bwd_args&) { return 1; }
  static __device__ __forceinline__ constexpr bool scale(const mgn_mlp_bwd_args&) { return true; }
  static __device__ __forceinline__ constexpr bool din_resid(const mgn_mlp_bwd_args&) { return true; }
};
__device__ __forceinline__ float ldfu(const float* p) {  // untracked scalar-per-lane load (see ld2u)
  float v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ u32 ldwu(const uint32_t* p) {
  u32 v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
template <int TERMS, bool FRONT, int ACT, bool SEG = false, class SB = SbDyn>
__global__ void __launch_bounds__(256, 2) k_mlp_bwd_x6(const mgn_mlp_bwd_args a) {
  constexpr int HB = 8, H = 128;
  constexpr bool UT = SB::ST;  // static shape: unit loops unroll, operand loads are untracked (mgn_x6.inc, ld2u)
  static_assert(!UT || (!FRONT && !SEG && ACT == MGN_ACT_RELU), "static backward shape: plain ReLU chain only");
  const int NLL = SB::NL(a), NDIN = SB::n_din(a);
  const bool HAS_SCALE = SB::scale(a), HAS_DRESID = SB::din_resid(a);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* ring = (lds_char*)smem;
  lds_char* cst = ring + X6_RING * X6_QBYTES;                        // scale
  float* lds = (float*)(smem + X6_RING * X6_QBYTES + 512);           // [4 waves][nslot][H]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const unsigned lane16 = 16u * lane;
  const int nslot = NLL + 1;  // slots of red_ws: db[0..NL-1], dscale
  // requested column sums, packed: LDS slot of red_ws slot l = number of requested slots below l
  const bool hb0 = a.db[0] != nullptr, hb1 = a.db[1] != nullptr, hb2 = a.db[2] != nullptr, hb3 = a.db[3] != nullptr;
  const bool hsc = HAS_SCALE && a.dscale != nullptr;
  auto lds_slot = [&](int l) -> int { return (int)(hb0 && l > 0) + (int)(hb1 && l > 1) + (int)(hb2 && l > 2) + (int)(hb3 && l > 3); };
  auto slot_used = [&](int l) -> bool { return (l == NLL) ? hsc : pick4(hb0, hb1, hb2, hb3, l); };
  const int nused = lds_slot(NLL) + (hsc ? 1 : 0);
  float* lds_w = lds + wv * nused * H;
  for (int i = lane; i < nused * H; i += 64) lds_w[i] = 0.f;
  for (int i = threadIdx.x; i < H; i += 256)
    ((__attribute__((address_space(3))) float*)cst)[i] = HAS_SCALE ? a.scale[i] : 0.f;
  const long ntiles = (a.M + 63) / 64;
  const TileWalk tw = tile_walk(ntiles);
  long tile = tw.first;
  const long my_tiles = tw.count;
  // optional front stage (fusion of the dX launch of round i with the node chain of round i-1):
  //   dY[m] = front_resid[m] + sum_p Wfront_p . front_src[p][m]   (stored to front_out)
  // its n_front units lead the stream; `src_rows` is what the tile's first operand rows are
  const int nf = FRONT ? a.n_front : 0;
  const int G = nf + (NLL - 1) + NDIN;
  const char *U0 = (const char*)a.wpk[0], *U1 = (const char*)a.wpk[1], *U2 = (const char*)a.wpk[2], *U3 = (const char*)a.wpk[3];
  const char *U4 = (const char*)a.wpk[4], *U5 = (const char*)a.wpk[5], *U6 = (const char*)a.wpk[6], *U7 = (const char*)a.wpk[7];
  const bool contig = x6_contig(U0, U1, U2, U3, U4, U5, U6, U7, G);
  const float *F0 = a.front_src[0], *F1 = a.front_src[1], *F2 = a.front_src[2];
  const float* fres = a.front_resid;
  float* fout = a.front_out;
  const float* src_rows = (nf > 0) ? F0 : a.dOut;          // rows that land in dz for the next tile
  const float* add_rows = (nf > 0) ? fres : a.dOut2;        // rows that land in pd2 (gathered by idx2 only without a front)
  const int32_t* add_idx = (nf > 0) ? nullptr : a.idx2;
  const uint32_t *Ms0 = a.Ms[0], *Ms1 = a.Ms[1], *Ms2 = a.Ms[2];
  const float *Zs0 = a.Zs[0], *Zs1 = a.Zs[1], *Zs2 = a.Zs[2];
  float *dZ0 = a.dZ[0], *dZ1 = a.dZ[1], *dZ2 = a.dZ[2], *dZ3 = a.dZ[3];
  float *db0 = a.db[0], *db1 = a.db[1], *db2 = a.db[2], *db3 = a.db[3];
  const float* dr0 = HAS_DRESID ? a.din_resid[0] : nullptr;
  float* dI0 = a.dIn[0];
  const unsigned ring0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring));

  constexpr int PPWB = (TERMS == 1) ? 2 : 6;   // 1 KB DMA pieces per wave and quarter (bf16 matrix mode: the leading piece only, as in the forward)
  QStream qs;
  qs.issued = 0, qs.total = my_tiles * 4 * G, qs.du = 0, qs.dq = 0, qs.dslot = 0, qs.cslot = 0, qs.young = 0;
  auto next_job = [&]() -> DmaQ {
    DmaQ j;
    const char* up = contig ? U0 + (size_t)qs.du * MGN_WPACK_BYTES : pick8(U0, U1, U2, U3, U4, U5, U6, U7, qs.du);
    j.su = (const char*)uniform_ptr((const float*)(up + qs.dq * X6_QBYTES + wv * (PPWB * 1024)));
    j.lds = ring0 + qs.dslot * X6_QBYTES + wv * (PPWB * 1024);
    j.on = qs.issued < qs.total;
    ++qs.issued;
    qs.dslot = (qs.dslot == X6_RING - 1) ? 0 : qs.dslot + 1;
    if (++qs.dq == 4) {
      qs.dq = 0;
      qs.du = (qs.du + 1 == G) ? 0 : qs.du + 1;
    }
    return j;
  };
  // dscale = sum_rows dY * U.  Per tile the 32 per-lane products are folded over the 16 rows of
  // the tile by a halving butterfly (each step a lane keeps one half of its values and hands the
  // other half to lane c ^ m): 2 running sums per lane instead of 32 -- the registers are needed
  // for operand prefetch.  Lane (c,g) ends up owning features 16*ib + 4g + r with
  // 4*ib + r = (c0<<4 | c1<<3 | c2<<2 | c3<<1) + {0,1}.
  float dsum2[2] = {0.f, 0.f};

  if (my_tiles > 0) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const DmaQ j0 = next_job();
#pragma unroll
      for (int i = 0; i < PPWB; ++i) dmaq_issue(j0, i, lane16);
    }
    auto rows_of = [&](long tl, long& mm, bool& valid) {
      const long m = (tl * 4 + wv) * 16 + c;
      valid = m < a.M;
      mm = valid ? m : a.M - 1;
    };
    long mm;
    bool valid;
    rows_of(tile, mm, valid);
    // dz: gradient rows -> the next tile's dOut rows (ReLU masks travel as one bit word per lane);
    // pu: U rows of this tile -> din residual rows -> the next tile's U rows; pd2: gathered dOut2 rows
    f32x4 dz[HB], acc[HB], pu[HB], pd2[HB];
    u32x4 xs[4][3];
    float prms;
    long r2n = 0;
    int r2u = 0;  // static shape: the NEXT tile's gather row, fetched (untracked) under the tile's first unit
    u32 mbits = 0;
    auto LD2 = [&](f32x4 (&dst)[8], const float* rowp, int s, int& n) {
      if constexpr (UT) ld2u(dst, rowp, s, n);
      else ld2(dst, rowp, s, n);
    };
    {
      const long r2 = (add_rows != nullptr) ? (add_idx ? (long)add_idx[mm] : mm) : 0;
      prms = HAS_SCALE ? ld1(a.R + mm) : 0.f;
#pragma unroll
      for (int kb = 0; kb < HB; ++kb) {
        dz[kb] = ld4(src_rows + mm * H + 4 * g + 16 * kb);
        pd2[kb] = (add_rows != nullptr) ? ld4(add_rows + r2 * H + 4 * g + 16 * kb) : f32x4{0.f, 0.f, 0.f, 0.f};
        pu[kb] = HAS_SCALE ? ld4(a.U + mm * H + 4 * g + 16 * kb) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    dma_drain();
    __syncthreads();  // scale visible, first two quarters landed

    auto run_unit = [&](auto late) {
#pragma unroll
      for (int jq = 0; jq < 4; ++jq) {
        __syncthreads();
        const DmaQ job = next_job();
        const int before = qs.young;
        qs.young = 0;
        int early = 0;
        gemm_q<TERMS, PPWB>(acc, xs[jq], ring + qs.cslot * X6_QBYTES, lane16, job, [&](int s) { late(jq, s, (s < 3) ? early : qs.young); });
        qs.cslot = (qs.cslot == X6_RING - 1) ? 0 : qs.cslot + 1;
        drain_allow(before + (job.on ? PPWB : 0) + early + qs.young);
      }
    };

    for (; tile < tw.end; tile += tw.stride) {
      const long ntile = tile + tw.stride;
      const bool has_next = ntile < tw.end;
      const bool wvalid = __builtin_amdgcn_readfirstlane((int)((tile * 4 + wv) * 16 < a.M));
      long mmn;
      bool validn;
      rows_of(has_next ? ntile : tile, mmn, validn);
      if (nf > 0) {  // ---- front stage: dY = resid + sum_p Wfront_p . rows_p
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) acc[ib] = pd2[ib];
        for (int p = 0; p < nf; ++p) {
          split_tile<TERMS, !FRONT && !SEG>(dz, xs);
          const float* nxt = (p == 0) ? F1 : F2;
          run_unit([&](int jq, int s, int& n) {
            if (jq == 0 && p + 1 < nf) ld2(dz, nxt + mm * H + 4 * g, s, n);
          });
        }
        if (fout != nullptr) {
          if (valid) {
#pragma unroll
            for (int ib = 0; ib < HB; ++ib) st4(fout + mm * H + 4 * g + 16 * ib, acc[ib]);
          }
          if (wvalid) qs.young += 8;
        }
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) dz[ib] = valid ? acc[ib] : f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) {
          // without a second gradient stream pd2 holds zeros only until a SiLU chain unit has parked pre-activation rows
          // in it (second and later tiles of a workgroup: node-row launches above 32 768 rows): add nothing then
          const f32x4 extra = (add_rows != nullptr) ? pd2[ib] : f32x4{0.f, 0.f, 0.f, 0.f};
          dz[ib] = valid ? dz[ib] + extra : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      // ---- dY, RMSNorm backward:  dz = g/(rms+eps) - u * <g,u> / (H*rms),  g = scale*dY
      if (HAS_SCALE) {
        float dot = 0.f;
        if (a.dscale != nullptr) {
          float v[32];
#pragma unroll
          for (int ib = 0; ib < HB; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * ib + r] = dz[ib][r] * pu[ib][r];
          fold_step<0>(v, c), fold_step<1>(v, c), fold_step<2>(v, c), fold_step<3>(v, c);
          dsum2[0] += v[0];
          dsum2[1] += v[1];
        }
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) {
          const f32x4 gg = *(lds_cf32x4*)(cst + 64 * ib + 16 * g) * dz[ib];
#pragma unroll
          for (int r = 0; r < 4; ++r) dot = fmaf(gg[r], pu[ib][r], dot);
          dz[ib] = gg;
        }
        dot = rowsum4(dot);
        const float rms = prms;
        const float inv = 1.0f / (rms + a.eps);
        const float k2 = (rms > 0.f) ? dot / ((float)H * rms) : 0.f;
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) dz[ib] = dz[ib] * inv - pu[ib] * k2;
      }
      // [r4] precision == 2 (bf16 matrix mode, two-byte rows): dZ[l] for l >= 1 -- read back by the weight gradients only -- is stored as
      // the packed leading pieces of its own split (the operand of the next input-gradient product), in the forward's packed
      // feature order (mgn_mlp_fwd_args.precision); dZ[0] stays fp32 (the scatter onto the nodes reads it)
      const bool d16 = (TERMS == 1) && a.precision >= 2;
      float* dzl_top = pick4(dZ0, dZ1, dZ2, dZ3, NLL - 1);
      const bool top16 = d16 && (NLL - 1 >= 1 || a.precision == 3);
      {
        float* dzl = dzl_top;
        if (dzl != nullptr && !top16) {
          if (valid) {
#pragma unroll
            for (int ib = 0; ib < HB; ++ib) st4(dzl + mm * H + 4 * g + 16 * ib, dz[ib]);
          }
          if (wvalid) qs.young += 8;
        }
        if (pick4(db0, db1, db2, db3, NLL - 1) != nullptr) {
          const f32x4(&dz1)[1][HB] = *(const f32x4(*)[1][HB]) & dz;
          colsum_to_lds_add<HB, 1>(lds_w + lds_slot(NLL - 1) * H, dz1, c, g);
        }
      }
      split_tile<TERMS, !FRONT && !SEG>(dz, xs);
      if (TERMS == 1 && dzl_top != nullptr && top16) {
        if (valid) {
#pragma unroll
          for (int pq = 0; pq < 4; ++pq)
            st4((float*)((char*)dzl_top + (size_t)(mm * H + 32 * pq + 8 * g) * 2), __builtin_bit_cast(f32x4, xs[pq][0]));
        }
        if (wvalid) qs.young += 4;
      }
      // prefetch of the next tile's rms / U rows / gathered dOut2 rows, riding under a unit
      auto pref = [&](int jq, int s, int& n) {
        if (jq == 1) {
          if (s == 0) {
            if (HAS_SCALE) {
              prms = ld1(a.R + mmn);
              n += 1;
            }
            r2n = mmn;
            if (add_rows != nullptr && add_idx != nullptr) {
              r2n = (long)add_idx[mmn];
              n += 1;
            }
          }
          if (HAS_SCALE) ld2(pu, a.U + mmn * H + 4 * g, s, n);
        } else if (jq == 2) {
          if (add_rows != nullptr) ld2(pd2, add_rows + r2n * H + 4 * g, s, n);
        }
      };
      // static shape: the same operands, untracked.  A step-3 load of quarter q is only ordered by the drain of
      // quarter q + 2, so the rows of quarter 2 go out in its first three steps; the gather row was fetched under
      // the tile's FIRST unit
      auto pref_u = [&](int jq, int s, int& n) {
        if (jq == 0) {
          if (s == 0) {
            prms = ldfu(a.R + mmn);
            n += 1;
          }
          ld2u(pu, a.U + mmn * H + 4 * g, s, n);
        } else if (jq == 1) {
          ld2u(pd2, add_rows + (long)landed(r2u) * H + 4 * g, s, n);
        } else if (jq == 2) {
          ld3u(dz, src_rows + mmn * H + 4 * g, s, n);  // steps 0..2 only: landed when the unit's last drain has passed
        }
      };
      // ---- chain units: dz_{l-1} = (W_l^T dz_l) masked by the ReLU bits of layer l's input
      auto chain_unit = [&](int k) {
        const int l = NLL - 1 - k;
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) acc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bool fetch_resid = (k == NLL - 2) && NDIN == 1 && HAS_DRESID;
        const bool pref_here = (k == NLL - 2) && NDIN == 0 && has_next;
        run_unit([&](int jq, int s, int& n) {
          if (ACT == MGN_ACT_SILU) {
            // pre-activation rows of this layer's input -> pd2 (free between the tile's first use and
            // the next tile's prefetch, which rides under the input-grad unit; n_din == 0 with
            // gathered dOut2 rows is kept off this kernel by the host)
            if (jq == 0) ld2(pd2, pick3(Zs0, Zs1, Zs2, l - 1) + mm * H + 4 * g, s, n);
          } else if (jq == 0 && s == 0) {  // ReLU mask bits of this lane's 32 features
            if constexpr (UT) mbits = ldwu(pick3(Ms0, Ms1, Ms2, l - 1) + mm * 4 + g);
            else mbits = *(__attribute__((address_space(1))) const u32*)(pick3(Ms0, Ms1, Ms2, l - 1) + mm * 4 + g);
            n += 1;
            if (UT && k == 0) {  // the next tile's gather row (used under the tile's last unit)
              if constexpr (UT) r2u = ldiu(add_idx + mmn);
              n += 1;
            }
          }
          if (fetch_resid) {  // residual rows of the input-grad unit
            if (jq == 1) LD2(pu, dr0 + mm * H + 4 * g, s, n);
          } else if (pref_here) {
            pref(jq, s, n);
          }
        });
        if (ACT == MGN_ACT_SILU) {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) dz[ib][r] = valid ? acc[ib][r] * dsilu_f(pd2[ib][r]) : 0.f;
        } else {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) dz[ib][r] = (valid && ((mbits >> (4 * ib + r)) & 1u)) ? acc[ib][r] : 0.f;
        }
        float* dzp = pick3(dZ0, dZ1, dZ2, l - 1);
        const bool low16 = d16 && (l - 1 >= 1 || a.precision == 3);   // (3: dZ[0] too -- read by mgn_segsum2_b16 and the weight gradients)
        if (dzp != nullptr && !low16) {
          if (valid) {
#pragma unroll
            for (int ib = 0; ib < HB; ++ib) st4(dzp + mm * H + 4 * g + 16 * ib, dz[ib]);
          }
          if (wvalid) qs.young += 8;
        }
        if (pick3(db0, db1, db2, l - 1) != nullptr) {
          const f32x4(&dz1)[1][HB] = *(const f32x4(*)[1][HB]) & dz;
          colsum_to_lds_add<HB, 1>(lds_w + lds_slot(l - 1) * H, dz1, c, g);
        }
        if (k + 1 < G || low16) split_tile<TERMS, !FRONT && !SEG>(dz, xs);
        if (TERMS == 1 && dzp != nullptr && low16) {
          if (valid) {
#pragma unroll
            for (int pq = 0; pq < 4; ++pq)
              st4((float*)((char*)dzp + (size_t)(mm * H + 32 * pq + 8 * g) * 2), __builtin_bit_cast(f32x4, xs[pq][0]));
          }
          if (wvalid) qs.young += 4;
        }
        if (SEG && l == 1) {
          // dZ[0] is complete (stored, split for the input-grad unit): its sum over the rows of every
          // destination node -- the backward scatter onto destinations -- by the forward's segmented scan;
          // dz is dead after this (the input-grad unit refills it with the next tile's rows)
          // (the run-end stores are not counted in qs.young: uncounted operations only make a drain over-wait)
          seg_scan_store(dz, valid ? a.seg_key[mm] : -1, (tile * 4 + wv), a.seg_rowptr, a.seg_out, a.seg_part, g);
        }
      };
      if constexpr (UT) {
#pragma unroll
        for (int k = 0; k < SB::NL(a) - 1; ++k) chain_unit(k);
      } else {
        for (int k = 0; k < NLL - 1; ++k) chain_unit(k);
      }
      // ---- input-grad unit (the last of the tile): dIn = resid + WT0 dz_0; the next tile's
      //      operands (dOut -> dz, U -> pu, dOut2 -> pd2) travel under it
      if (NDIN == 1) {
        if (dr0 == nullptr) {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib) acc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib) acc[ib] = pu[ib];
        }
        run_unit([&](int jq, int s, int& n) {
          if constexpr (UT) {
            pref_u(jq, s, n);  // unconditional statements: the last tile re-reads its own rows
          } else {
            if (jq == 0)
              ld2(dz, src_rows + mmn * H + 4 * g, s, n);
            else if (has_next)
              pref(jq, s, n);
          }
        });
        if (valid) {
#pragma unroll
          for (int ib = 0; ib < HB; ++ib) st4(dI0 + mm * H + 4 * g + 16 * ib, acc[ib]);
        }
        if (wvalid) qs.young += 8;
      }
      if (NDIN == 0 && has_next) {  // no input-grad unit to hide it under
#pragma unroll
        for (int kb = 0; kb < HB; ++kb) dz[kb] = ld4(src_rows + mmn * H + 4 * g + 16 * kb);
      }
      mm = mmn;
      valid = validn;
    }
  }
  // dscale: one cross-lane reduction per workgroup
  if (HAS_SCALE && a.dscale != nullptr) {
    const int i0 = ((c & 1) << 4) | ((c & 2) << 2) | (c & 4) | ((c & 8) >> 2);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = i0 + k;
      lds_w[lds_slot(NLL) * H + 16 * (i >> 2) + 4 * g + (i & 3)] = dsum2[k];
    }
  }
  __syncthreads();
  float* ws = (float*)a.red_ws + (size_t)blockIdx.x * nslot * H;
  for (int i = threadIdx.x; i < nslot * H; i += 256) {  // red_ws keeps its [NL + 1][H] layout; unrequested slots are not read
    const int l = i >> 7;
    if (slot_used(l)) {
      const int j = lds_slot(l) * H + (i & 127);
      ws[i] = ((lds[j] + lds[nused * H + j]) + lds[2 * nused * H + j]) + lds[3 * nused * H + j];
    }
  }
}

// ------------------------------------------------------------------- weight grads
// dW[j,k] = sum_m dZ[m,j] X[m,k] on the split-bf16 matrix path.  Same streaming skeleton as
// k_wgrad_lds (32-row tiles of A = dZ and B = X through LDS by DMA, double buffered, per-WG
// partials + k_wgrad_red), but one tile is ONE K = 32 MFMA step: lane (c,g) reads rows
// 8g..8g+7 of feature 16b + c (ds_read_b32, N-layout), splits the 8 values into bf16x3 and
// packs them -- that IS the A (dZ^T) / B (X) operand.  Wave wv owns the 4 x 4 block of
// 16x16 outputs jb in 4*(wv>>1).., kb in 4*(wv&1)..: 64 values to split per tile for 96 MFMAs.
// Tile image: row r at byte 512*r, 16-byte chunk p holds global chunk p ^ (4*((r>>3)&1)):
// rows 8g+t of even / odd g sit 16 banks apart, so the 32 lanes of a ds_read_b32 group
// (two values of g) never share a bank.
// [r3] What bounds it (tools/kbench_wgrad.py, the four E-row jobs of a round + k_wgrad_red, bench shape): 191 us shipped; a build
// without the splits 156 us, with one MFMA term of six 146 us, with neither 145 us -- either half of the arithmetic hides under
// the tile stream, both together do not: ~500 VALU + 96 MFMA instructions per tile and wave from two waves per SIMD.  Tried and
// measured neutral (190.8-199 us): two tiles in flight per workgroup (refill of the buffer just read, one more barrier), the refill's
// eight DMA instructions spread under the MFMA terms, per-lane DMA offsets hoisted out of the tile loop.  Not bytes in flight, then;
// the remaining lever is to split each operand block once per workgroup instead of once per wave pair (48 KB of LDS that two
// workgroups per CU do not have).
// [r4] the same for rows stored as bf16 (256 bytes; the two-byte saves of precision == 2): a 32-row tile is 8 pieces of 4 rows, two per
// wave; 16-byte chunk p of row r holds global chunk p ^ (4 * ((r >> 3) & 1)), so the 2-byte reads of rows 8g + t (lane groups of 32
// = two values of g) fall 64 bytes apart (dma_op of k_wgrad_x6)
__device__ __forceinline__ void dma_row_piece8(const float* __restrict__ X, long row0, long M, unsigned lds0, int wv, int lane, int i) {
  const int q = 4 * wv + i;
  const int r = 2 * q + (lane >> 5);
  long row = row0 + r;
  row = row < M ? row : M - 1;  // tail rows are masked before the MFMA
  const int gch = (lane & 31) ^ (4 * ((r >> 3) & 1));
  const unsigned voff = (unsigned)((row - row0) * 512 + 16 * gch);
  glds16(uniform_ptr(X + row0 * 128), voff, lds0 + q * 1024);
}

// 8 fp32 (consecutive rows of one feature) -> three packed operands, level by level
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& p1, u32x4& p2, u32x4& p3) {
  float ra[4], rb[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) p1[h] = pk_bf16(v[2 * h], v[2 * h + 1]);
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    ra[h] = v[2 * h] - bf_lo(p1[h]);
    rb[h] = v[2 * h + 1] - bf_hi(p1[h]);
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) p2[h] = pk_bf16(ra[h], rb[h]);
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    ra[h] -= bf_lo(p2[h]);
    rb[h] -= bf_hi(p2[h]);
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) p3[h] = pk_bf16(ra[h], rb[h]);
}

// [r4] The same remainders-from-the-matrix-pipe trick as split_pair_mfma for the weight-gradient operands.  A lane's 8 values
// (rows 8g..8g+7 of one feature) ARE the B operand of a K = 32 MFMA; seen as two 16 x 16 tiles in the C/D layout (rows
// 8g'+0..3 and rows 8g'+4..7, column = the feature) they are also its C input, so  v - bf16(v) = Sel . piece + v  with
// Sel_h[i][k] = -1 where k = 8 (i >> 2) + 4 h + (i & 3): lane (i, g) holds -1 at element 4 h + (i & 3) when g == i >> 2.
// 12 conversions + 4 MFMAs per block instead of 44 VALU instructions.  Used by the producers of k_wgrad_pc; k_wgrad_x6 keeps the
// vector form split8 (the matrix-pipe form made it matrix-bound where it was VALU-bound: DESIGN.md section 9).
struct WgSel {
  u32x4 s0, s1;
};
__device__ __forceinline__ WgSel wg_sel(int c, int g) {
  WgSel S;
  const u32 m1 = 0xbf80u;  // bf16(-1.0)
  const bool on = (g == (c >> 2));
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    u32 w0 = 0, w1 = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = 2 * d + h;  // element e of the lane's 8
      if (on && e == (c & 3)) w0 |= m1 << (16 * h);
      if (on && e == 4 + (c & 3)) w1 |= m1 << (16 * h);
    }
    S.s0[d] = w0, S.s1[d] = w1;
  }
  return S;
}

template <int TERMS>
__global__ void __launch_bounds__(256, 2) k_wgrad_x6(const WgradLaunch L) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* sm = (lds_char*)smem;  // [2 buffers][A tile | B tile]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  int j = 0;
  while (j + 1 < L.njobs && (int)blockIdx.x >= L.wg0[j + 1]) ++j;
  const mgn_wgrad_job J = L.job[j];
  const int nwg = L.wg0[j + 1] - L.wg0[j];
  const int wg = blockIdx.x - L.wg0[j];
  const long ntiles = (J.M + WG_TILE_ROWS - 1) / WG_TILE_ROWS;
  const long t0 = ntiles * wg / nwg, t1 = ntiles * (wg + 1) / nwg;
  const unsigned sm0 = __builtin_amdgcn_readfirstlane(lds_addr_of(sm));
  const int jb0 = 4 * (wv >> 1), kb0 = 4 * (wv & 1);
  // (unused since the matrix-pipe split left this kernel for k_wgrad_pc, and dead after optimisation -- but without the line hipcc
  // swaps two scalar instructions of k_wgrad_x6<1>; it goes with the next change that alters this kernel's code anyway)
  const WgSel wsel = wg_sel(c, g);

  f32x4 acc[4][4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc[jj][kk] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cs[4] = {0.f, 0.f, 0.f, 0.f};  // waves with kb0 == 0: column sums of A (bias gradient)
  const bool want_db = (J.db != nullptr) && ((wv & 1) == 0);
  // lane (c,g): row 8g + t, feature 16b + c  ->  byte g*4096 + t*512 + 64*(b ^ (g&1)) + 4c
  const int lb = g * 4096 + 4 * c;
  const int gx = g & 1;
  // (readfirstlane: the flags must be PROVABLY uniform -- the two DMA forms are merged into one asm statement with selected operands)
  const bool b16 = (TERMS == 1) && __builtin_amdgcn_readfirstlane(J.ldb) < 0;   // B = two-byte saves of the forward (rows of 256 bytes in its packed feature order)
  const bool a16 = (TERMS == 1) && __builtin_amdgcn_readfirstlane(J.lda) < 0;   // A = two-byte dZ rows of the backward chain (same order)
  // one DMA statement per operand whatever its row type (fp32 rows: 4 pieces of 2 rows per wave, bf16 rows: 2 pieces of 4 rows): the
  // row type only selects uniform scalars, so the "s" operands of the asm stay scalar
  auto dma_op = [&](const float* X, bool bf, long row0, unsigned lds0, int i) {
    const int q = (bf ? 2 : 4) * wv + i;
    const int r = bf ? 4 * q + (lane >> 4) : 2 * q + (lane >> 5);
    long row = row0 + r;
    row = row < J.M ? row : J.M - 1;  // tail rows are masked before the MFMA
    const int gch = (bf ? (lane & 15) : (lane & 31)) ^ (4 * ((r >> 3) & 1));
    const unsigned voff = (unsigned)((row - row0) * (bf ? 256 : 512) + 16 * gch);
    const char* base = (const char*)X + row0 * (bf ? 256 : 512);
    const unsigned ldst = __builtin_amdgcn_readfirstlane(lds0 + q * 1024);
    if (i < (bf ? 2 : 4)) glds16(uniform_ptr((const float*)base), voff, ldst);
  };
  auto dma_tile = [&](long row0, unsigned lds_a) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dma_op(J.A, a16, row0, lds_a, i);
      dma_op(J.B, b16, row0, lds_a + WG_TILE_BYTES, i);
    }
  };
  if (t0 < t1) dma_tile(t0 * WG_TILE_ROWS, sm0);
  for (long tile = t0; tile < t1; ++tile) {
    const int buf = (int)((tile - t0) & 1);
    dma_drain();
    __syncthreads();  // tile landed; the other buffer is free again
    const bool more = tile + 1 < t1;
    const unsigned nb0 = sm0 + (buf ^ 1) * 2 * WG_TILE_BYTES;
    lds_char* ta = sm + buf * 2 * WG_TILE_BYTES;
    lds_char* tb = ta + WG_TILE_BYTES;
    if (more) dma_tile((tile + 1) * WG_TILE_ROWS, nb0);  // next tile's DMA rides under the splits and MFMAs
    // rows past M (the DMA clamps them to row M-1) must not contribute: only a job's last tile
    const int rows_left = (int)(J.M - tile * WG_TILE_ROWS);
    u32x4 ap[4][3], bp[4][3];
    // operand blocks two at a time: read 2 x 8 values from the tile image, split them into their bf16x3 pieces
    auto take = [&](lds_char* img, int blk0, bool is_a, u32x4 (&out)[4][3], int o) {
      float v[2][8];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int t = 0; t < 8; ++t)
          v[q][t] = *(__attribute__((address_space(3))) const float*)(img + lb + t * 512 + 64 * ((blk0 + o + q) ^ gx));
      if (is_a) {
        if (rows_left < WG_TILE_ROWS) {
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const float keep = (8 * g + t < rows_left) ? 1.f : 0.f;
#pragma unroll
            for (int q = 0; q < 2; ++q) v[q][t] *= keep;
          }
        }
        if (want_db) {
#pragma unroll
          for (int q = 0; q < 2; ++q)
            cs[o + q] += ((v[q][0] + v[q][1]) + (v[q][2] + v[q][3])) + ((v[q][4] + v[q][5]) + (v[q][6] + v[q][7]));
        }
      }
      split8(v[0], out[o][0], out[o][1], out[o][2]);
      split8(v[1], out[o + 1][0], out[o + 1][1], out[o + 1][2]);
      __builtin_amdgcn_sched_barrier(0);  // (more pairs in flight cost registers: the kernel spills)
    };
    // bf16 rows: the eight values of a lane (rows 8g + t of one feature) are read as 2-byte halves straight into the packed operand
    auto take16 = [&](lds_char* img, int blk0, bool is_a, u32x4 (&out)[4][3]) {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int kb = blk0 + o;
        const int pos = 2 * (32 * (kb >> 1) + 8 * (c >> 2) + 4 * (kb & 1) + (c & 3));   // byte of feature 16 kb + c in the packed row
        lds_char* base = img + g * 2048 + 16 * ((pos >> 4) ^ (4 * gx)) + (pos & 15);
        u32x4 w;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const u32 lo = *(__attribute__((address_space(3))) const uint16_t*)(base + (2 * h) * 256);
          const u32 hi = *(__attribute__((address_space(3))) const uint16_t*)(base + (2 * h + 1) * 256);
          w[h] = lo | (hi << 16);
        }
        if (is_a) {
          if (rows_left < WG_TILE_ROWS) {   // rows past M must not contribute
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              const int r0_ = 8 * g + 2 * h;
              w[h] = (r0_ >= rows_left) ? 0u : ((r0_ + 1 >= rows_left) ? (w[h] & 0xffffu) : w[h]);
            }
          }
          if (want_db) cs[o] += ((bf_lo(w[0]) + bf_hi(w[0])) + (bf_lo(w[1]) + bf_hi(w[1]))) + ((bf_lo(w[2]) + bf_hi(w[2])) + (bf_lo(w[3]) + bf_hi(w[3])));
        }
        out[o][0] = w, out[o][1] = w, out[o][2] = w;   // (one term: only the leading piece is multiplied)
      }
    };
    if (a16) {
      take16(ta, jb0, true, ap);
    } else {
      take(ta, jb0, true, ap, 0);
      take(ta, jb0, true, ap, 2);
    }
    if (b16) {
      take16(tb, kb0, false, bp);
    } else {
      take(tb, kb0, false, bp, 0);
      take(tb, kb0, false, bp, 2);
    }
    // six terms, smallest first; 16 independent accumulators per term
#pragma unroll
    for (int term = (TERMS == 1 ? 5 : 0); term < 6; ++term) {
      const int pa = (term == 0) ? 2 : (term == 1) ? 0 : (term == 2 || term == 3) ? 1 : 0;
      const int pb = (term == 0) ? 0 : (term == 1) ? 2 : (term == 2) ? 1 : (term == 3) ? 0 : (term == 4) ? 1 : 0;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc[jj][kk] = MFMA_BF(ap[jj][pa], bp[kk][pb], acc[jj][kk]);
    }
  }
  float* P = L.partial + (size_t)blockIdx.x * (128 * 128 + 128);
  if (want_db) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float v = rowsum4(cs[jj]);
      if (g == 0) P[128 * 128 + 16 * (jb0 + jj) + c] = v;
    }
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int q = 0; q < 4; ++q) P[(16 * (jb0 + jj) + 4 * g + q) * 128 + 16 * (kb0 + kk) + c] = acc[jj][kk][q];
}

// ------------------------------------------------------------------- [r5] weight grads, producer / consumer form
// Same job (dW = dZ^T X over 32-row tiles, six bf16 terms, per-workgroup partials + k_wgrad_red) as k_wgrad_x6, re-cut so that
// every operand value is split into its bf16x3 pieces ONCE per workgroup (k_wgrad_x6: once per wave that multiplies it = twice;
// 5.3 vector instructions per MFMA, r04_pmc_stall_counters) and so that the waves that issue memory never wait for the matrix pipe:
//   * 512 threads, ONE workgroup per CU.  Waves 0-3 are PRODUCERS, waves 4-7 CONSUMERS (one of each per SIMD).
//   * A producer owns 16 rows x 128 features of A (waves 0, 1) or B (waves 2, 3) of every tile: lane (rg, q) loads the 16 bytes
//     [4q, 4q + 4) of rows 8g + 0..7 (g = 2 * half + rg) with eight global_load_dwordx4 -- each instruction is two whole
//     512-byte rows, row-contiguous (17 TA cycles against the 64 of a T-layout tile, r04_ta_probe) -- and then HOLDS the
//     transposed operand: for each of its 4 features the 8 consecutive rows that are one lane's K-slice of the 16x16x32 MFMA.
//     split8 (44 vector instructions per 8 values) and three ds_write_b128 per feature put the pieces where a consumer lane reads
//     them.  Two tiles of rows are in flight per producer (64 registers: producers have no accumulators), so a CU keeps 64 KB
//     of loads outstanding whatever the consumers do.
//   * A consumer owns a 64 x 64 quadrant of dW (4 x 4 accumulator blocks): 24 ds_read_b128 + 96 MFMAs per tile, nothing else.
//   * LDS: THREE piece images of 48 KB ([A | B][block 8][piece 3][g 4][16 slots of 16 B]) and ONE s_barrier per tile.  Between
//     barriers k - 1 and k the producers fill image k % 3 (tile k), the consumers multiply tile k - 2 out of registers and re-load
//     every operand register from image (k - 1) % 3 as soon as its last MFMA of tile k - 2 has been issued (the term order
//     (a1,b3) (a1,b2) (a2,b2) (a1,b1) (a2,b1) (a3,b1) leaves every piece at least two terms = 512 matrix cycles between its
//     last use and its next first use), so the matrix pipe never waits for an LDS read and a consumer needs no wait at its
//     barrier: the image it reads now is written again two barriers later, after the MFMAs that consumed the reads.
//     Slot of operand lane c in its 256-byte row:
//     c ^ ((c >> 3) << 1) ^ (block & 1) -- the 8-lane groups of a ds_write_b128 (lanes q = 8k .. 8k + 7: two blocks x four
//     16-byte column groups) then cover the 8 slots of a 128-byte bank row, and the 16-lane groups of a ds_read_b128 still see
//     16 distinct slots (the swizzle permutes within {0-3}, {4-7}, {8-11}, {12-15}).
//   * Measured on the way (timing-experiment builds, bench shape, first version with two images and a consumer that read all 24 operand
//     vectors after each barrier: 165 us against 183 us for k_wgrad_x6): without the splits 156-163 us, with two of six terms
//     138 us, with cache-resident rows 123 us, with neither splits nor terms 137 us (the row stream + exchange alone), with none
//     of the three 77 us.
// Full 128 x 128 jobs with fp32 rows only (lda = ldb = 128); the bf16-row jobs of the bf16 matrix mode stay on k_wgrad_x6<1>.
#define WPC_IMG 49152
#define WPC_NIMG 3
#define WPC_LDS_BYTES (WPC_NIMG * WPC_IMG + 64)
#ifdef MGN_TIMELINE
// debug build only (tools/timeline_wpc.py): s_memtime stamps of wave 0 (a producer of A) and wave 4 (a consumer) of workgroup 0
__device__ unsigned long long g_wpc_tl[2][2048];
__device__ int g_wpc_tln[2];
__device__ unsigned long long g_wpc_wg[512][2];   // s_memrealtime at the start / end of every workgroup
#define WPC_TL_DECL()                                   \
  int tl_n_ = 0;                                        \
  const bool tl_on_ = blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == 256)
#define WPC_STAMP(tag)                                                                                                  \
  do {                                                                                                                  \
    if (tl_on_ && tl_n_ < 2048) g_wpc_tl[threadIdx.x >> 8][tl_n_++] = (__builtin_readcyclecounter() << 8) | (tag);      \
  } while (0)
#define WPC_TL_DUMP()                               \
  do {                                              \
    WPC_STAMP(9);                                   \
    if (tl_on_ && tl_n_ < 2048) g_wpc_tl[threadIdx.x >> 8][tl_n_++] = (__builtin_amdgcn_s_memrealtime() << 8) | 8; \
    if (tl_on_) g_wpc_tln[threadIdx.x >> 8] = tl_n_; \
  } while (0)
extern "C" int mgn_debug_wpc_wgtimes(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wpc_wg), sizeof(unsigned long long) * 512 * 2) != hipSuccess;
}
extern "C" int mgn_debug_wpc_timeline(unsigned long long* out, int* n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wpc_tl), sizeof(unsigned long long) * 2 * 2048) != hipSuccess) return 1;
  return hipMemcpyFromSymbol(n, HIP_SYMBOL(g_wpc_tln), sizeof(int) * 2) != hipSuccess;
}
#else
#define WPC_TL_DECL() ((void)0)
#define WPC_STAMP(tag) ((void)0)
#define WPC_TL_DUMP() ((void)0)
#endif
__device__ __forceinline__ void wpc_barrier() {   // producers: their LDS writes have landed before the barrier publishes them
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void wpc_barrier_c() {  // consumers: reads in flight may cross it (see the image rotation above)
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

__global__ void __launch_bounds__(512, 2) k_wgrad_pc(const WgradLaunch L) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* sm = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int j = 0;
  while (j + 1 < L.njobs && (int)blockIdx.x >= L.wg0[j + 1]) ++j;
  const mgn_wgrad_job J = L.job[j];
  const int nwg = L.wg0[j + 1] - L.wg0[j];
  const int wg = blockIdx.x - L.wg0[j];
  const long ntiles = (J.M + WG_TILE_ROWS - 1) / WG_TILE_ROWS;
  // tiles of this workgroup, by local index k in [0, n): interleaved (tile = wg + k * nwg: at any moment the workgroups of a job read
  // one contiguous window of the operand rows, as a grid-stride copy does -- every memory channel carries the same share)
  const long t0 = 0, t1 = (ntiles - wg + nwg - 1) / nwg;
  auto gtile = [&](long k) { return (long)wg + k * nwg; };
  const bool has_last = t1 > 0 && gtile(t1 - 1) == ntiles - 1;
  float* P = L.partial + (size_t)blockIdx.x * (128 * 128 + 128);
  WPC_TL_DECL();
#ifdef MGN_TIMELINE
  if (tl_on_) g_wpc_tl[threadIdx.x >> 8][tl_n_++] = (__builtin_amdgcn_s_memrealtime() << 8) | 8;
  WPC_STAMP(7);
  if (threadIdx.x == 0 && blockIdx.x < 512) g_wpc_wg[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
#endif

  if (wv < 4) {
    // ------------------------------------------------------------ producer
    __builtin_amdgcn_s_setprio(1);  // producers: their loads / splits / writes go first, a consumer needs one issue slot per 16 cycles
    const int mat = wv >> 1, half = wv & 1;
    const int rg = lane >> 5, q = lane & 31;
    const int g = 2 * half + rg;
    const float* X = mat ? J.B : J.A;
    const int b = q >> 2;
    const int s = (((q >> 1) & 1) << 1) | (b & 1);
    lds_char* wa[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) wa[e] = sm + ((mat * 8 + b) * 3) * 1024 + g * 256 + 64 * (q & 3) + 16 * (e ^ s);
    const bool want_db = (mat == 0) && (J.db != nullptr);
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    f32x4 raw0[8], raw1[8], raw2[8], raw3[8];
    const WgSel wsel = wg_sel(lane & 15, lane >> 4);
    // The pipelined loop runs over FULL tiles only and ALWAYS issues eight loads per tile (past the range it re-reads the last
    // full tile): the compiler counts the operations in flight, and a second load path or a conditionally issued group turns
    // every wait of the loop into vmcnt(~0) -- the two-tile prefetch would collapse (seen in the ISA).  A job's ragged last
    // tile is one un-pipelined step after the loop.
    const long tf = (has_last && (J.M % WG_TILE_ROWS) != 0) ? t1 - 1 : t1;
    auto load_tile = [&](long tile_, f32x4 (&raw)[8]) {
      const long kk = tile_ < tf ? tile_ : tf - 1;
      const long tile = gtile(kk);
      const float* p = X + (tile * WG_TILE_ROWS + 8 * g) * 128 + 4 * q;
#pragma unroll
      for (int i = 0; i < 8; ++i) raw[i] = ld4(p + i * 128);
    };
    auto process = [&](f32x4 (&raw)[8], int buf) {
      if (want_db) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          cs[e] += ((raw[0][e] + raw[1][e]) + (raw[2][e] + raw[3][e])) + ((raw[4][e] + raw[5][e]) + (raw[6][e] + raw[7][e]));
      }
      WPC_STAMP(1);
      typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
      // the four features of a lane stage by stage (the matrix-pipe split of wg_sel, four times, interleaved: left to the compiler
      // they run one after the other, each a chain of conversion -> MFMA -> conversion -> MFMA -> conversion that waits for the shared matrix pipe
      // twice: 1440 cycles per tile in the s_memtime timeline)
      f32x4 r0[4], r1[4];
      u32x4 p1[4], p2[4], p3[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r0[e] = f32x4{raw[0][e], raw[1][e], raw[2][e], raw[3][e]};
        r1[e] = f32x4{raw[4][e], raw[5][e], raw[6][e], raw[7][e]};
        p1[e] = u32x4{pk_bf16(raw[0][e], raw[1][e]), pk_bf16(raw[2][e], raw[3][e]), pk_bf16(raw[4][e], raw[5][e]), pk_bf16(raw[6][e], raw[7][e])};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) r0[e] = MFMA_BF(wsel.s0, p1[e], r0[e]), r1[e] = MFMA_BF(wsel.s1, p1[e], r1[e]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lds_char* d = wa[e] + buf;
        *(lds_u32x4*)(d) = p1[e];
        p2[e] = u32x4{pk_bf16(r0[e][0], r0[e][1]), pk_bf16(r0[e][2], r0[e][3]), pk_bf16(r1[e][0], r1[e][1]), pk_bf16(r1[e][2], r1[e][3])};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) r0[e] = MFMA_BF(wsel.s0, p2[e], r0[e]), r1[e] = MFMA_BF(wsel.s1, p2[e], r1[e]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lds_char* d = wa[e] + buf;
        *(lds_u32x4*)(d + 1024) = p2[e];
        p3[e] = u32x4{pk_bf16(r0[e][0], r0[e][1]), pk_bf16(r0[e][2], r0[e][3]), pk_bf16(r1[e][0], r1[e][1]), pk_bf16(r1[e][2], r1[e][3])};
        *(lds_u32x4*)(d + 2048) = p3[e];
      }
    };
    // four row sets: the loads of tile k + 3 are issued BEFORE tile k is split (they do not queue behind ~1500 cycles of splits),
    // into the set tile k - 1 left; the image index (k % 3) is a run-time offset
    int img = 0;
    auto next_img = [&]() { img = (img == (WPC_NIMG - 1) * WPC_IMG) ? 0 : img + WPC_IMG; };
    if (t0 < tf) {
      load_tile(t0, raw0);
      __builtin_amdgcn_sched_barrier(0);  // (the groups must BE issued in this order, or the loop's waits are counted for another one)
      load_tile(t0 + 1, raw1);
      __builtin_amdgcn_sched_barrier(0);
      load_tile(t0 + 2, raw2);
      __builtin_amdgcn_sched_barrier(0);
      long tile = t0;
#define WPC_STEP(cur, nxt, ahead)            \
  WPC_STAMP(0);                              \
  load_tile(tile + ahead, nxt);              \
  __builtin_amdgcn_sched_barrier(0);         \
  WPC_STAMP(3);                              \
  process(cur, img);                         \
  WPC_STAMP(2);                              \
  next_img();                                \
  wpc_barrier()
      for (; tile + 3 < tf; tile += 4) {
        WPC_STEP(raw0, raw3, 3);
        WPC_STEP(raw1, raw0, 4);
        WPC_STEP(raw2, raw1, 5);
        WPC_STEP(raw3, raw2, 6);
      }
      // (up to three tiles left; raw0..raw2 hold them: after a full round the sets are back in place)
      if (tile < tf) {
        process(raw0, img);
        next_img();
        wpc_barrier();
      }
      if (tile + 1 < tf) {
        process(raw1, img);
        next_img();
        wpc_barrier();
      }
      if (tile + 2 < tf) {
        process(raw2, img);
        next_img();
        wpc_barrier();
      }
    }
    if (tf < t1) {  // the ragged tile: rows past M read row M - 1; A's are zeroed
      const long r0 = gtile(tf) * WG_TILE_ROWS + 8 * g;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        long r = r0 + i;
        r = r < J.M ? r : J.M - 1;
        raw0[i] = ld4(X + r * 128 + 4 * q);
      }
      if (mat == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (r0 + i >= J.M) raw0[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      process(raw0, img);
      wpc_barrier();
    }
    // bias gradient: lanes (rg = 0, 1) x waves (half = 0, 1) hold partial column sums of features 4q .. 4q + 3
    wpc_barrier();  // (consumers are past their last read: the images are free)
    if (mat == 0) {
      typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
      *(lds_f32x4*)(sm + (g * 128 + 4 * q) * 4) = cs;
    }
    wpc_barrier();
    if (want_db && wv == 0) {
      typedef __attribute__((address_space(3))) const float lds_cfloat;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int f = lane + 64 * h;
        lds_cfloat* r = (lds_cfloat*)sm + f;
        P[128 * 128 + f] = (r[0] + r[128]) + (r[256] + r[384]);
      }
    }
  } else {
    // ------------------------------------------------------------ consumer
    const int cw = wv - 4;
    const int c = lane & 15, g = lane >> 4;
    const int jb0 = 4 * (cw >> 1), kb0 = 4 * (cw & 1);
    f32x4 acc[4][4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) acc[jj][kk] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int sl0 = c ^ ((c >> 3) << 1);
    // read addresses: image + block * 3072 + piece * 1024 + g * 256 + 16 * (sl0 ^ (block & 1))
    lds_char* ra[2] = {sm + (jb0 * 3) * 1024 + g * 256 + 16 * sl0, sm + (jb0 * 3) * 1024 + g * 256 + 16 * (sl0 ^ 1)};
    lds_char* rb[2] = {sm + ((8 + kb0) * 3) * 1024 + g * 256 + 16 * sl0, sm + ((8 + kb0) * 3) * 1024 + g * 256 + 16 * (sl0 ^ 1)};
    u32x4 ap[4][3], bp[4][3];
    auto rdA = [&](int p, int img) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) ap[jj][p] = *(lds_cu32x4*)(ra[jj & 1] + img + jj * 3072 + p * 1024);
    };
    auto rdB = [&](int p, int img) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) bp[kk][p] = *(lds_cu32x4*)(rb[kk & 1] + img + kk * 3072 + p * 1024);
    };
    auto term = [&](int pa, int pb) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc[jj][kk] = MFMA_BF(ap[jj][pa], bp[kk][pb], acc[jj][kk]);
    };
    const long n = t1 - t0;
    if (n > 0) {
      wpc_barrier_c();   // image 0 = tile 0
      rdA(0, 0), rdB(2, 0), rdB(1, 0), rdA(1, 0), rdB(0, 0), rdA(2, 0);
      int img = 0;
      for (long k = 1; k < n; ++k) {
        img = (img == (WPC_NIMG - 1) * WPC_IMG) ? 0 : img + WPC_IMG;
        WPC_STAMP(1);
        wpc_barrier_c();   // image k % 3 = tile k; the registers hold tile k - 1 (the order of the accumulation does not matter
                           // for accuracy here: the accumulators carry the sums of all earlier tiles)
        WPC_STAMP(0);
        // (pinned: left alone, the scheduler sinks all 24 reads below the MFMAs -- to the end of the iteration, in front of the barrier)
#define WPC_PIN() __builtin_amdgcn_sched_barrier(0)
        term(0, 2);
        WPC_PIN();
        rdB(2, img);
        WPC_PIN();
        term(0, 1);
        term(1, 1);
        WPC_PIN();
        rdB(1, img);
        WPC_PIN();
        term(0, 0);
        WPC_PIN();
        rdA(0, img);
        WPC_PIN();
        term(1, 0);
        WPC_PIN();
        rdA(1, img);
        WPC_PIN();
        term(2, 0);
        WPC_PIN();
        rdA(2, img);
        rdB(0, img);
      }
      term(0, 2);
      term(0, 1), term(1, 1), term(0, 0), term(1, 0);
      term(2, 0);
    }
    wpc_barrier();
    wpc_barrier();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) P[(16 * (jb0 + jj) + 4 * g + qq) * 128 + 16 * (kb0 + kk) + c] = acc[jj][kk][qq];
  }
  WPC_TL_DUMP();
#ifdef MGN_TIMELINE
  if (threadIdx.x == 0 && blockIdx.x < 512) g_wpc_wg[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
}
