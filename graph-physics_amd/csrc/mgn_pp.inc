// "Ping-pong" generation of the split-bf16 edge update (included by mgn_kernels.hip after mgn_x6.inc).
//
// Why.  In the x6 generation a CU runs two independent 4-wave workgroups; each wave alternates GEMM quarters (48 MFMAs)
// with everything else (ReLU, bf16x3 split, RMSNorm, segmented scan, row loads / stores) and the hardware is left to
// interleave the two waves of a SIMD.  Measured (DESIGN 4.2, 4.6): the matrix pipe is 26-38 % busy, 58 % of the wave
// cycles are issue stalls -- the two waves are in their GEMM parts together and in their non-GEMM parts together.
//
// Here ONE 8-wave workgroup owns the CU and the alternation is explicit: waves 0-3 (group P) and waves 4-7 (group Q)
// sit pairwise on the same SIMDs (a workgroup's waves are dealt to the SIMDs cyclically, so wave i and wave i + 4 share
// one).  Time is cut into slots by s_barrier; in every slot ONE group runs a GEMM quarter at full matrix rate and the
// other does its non-GEMM work ("free slot") under it -- Q lags P by exactly one slot:
//
//     slot        2j          2j+1         2j+2         2j+3
//     P        C(j)         F(j)         C(j+1)       F(j+1)          C = 48 MFMAs on quarter j of the weight stream
//     Q        F(j-1)       C(j)         F(j)         C(j+1)          F = the wave's other work, cut into 16 pieces per tile
//
// The non-GEMM work of a 16-row tile is ~1100 VALU instructions against 16 x 48 MFMAs; spread evenly over the tile's 16
// free slots (the split of K-slice jq+1 happens in the free slot before quarter jq+1: "lazy split"; the RMSNorm / residual
// / segmented scan of tile t run in the free slots of tile t+1's first unit) a free slot needs 45-200 instructions and
// always ends before the partner's quarter does, so the matrix pipe sees back-to-back quarters.
//
// Weight stream: the same packed quarters as the x6 kernels (mgn_wpack), ring of 3 in LDS.  Quarter j is computed by P in
// slot 2j and by Q in slot 2j+1; Q's free slot F(j) (slot 2j+2) re-fills the ring slot it has just read with quarter j+3
// (6 x 1 KB LDS-DMA per wave), drains it at the end of F(j+1), and the barrier after that publishes it: two slots before
// P pre-loads its first fragments.  Every free slot ends with a COUNTED vmcnt: everything issued before this slot has
// landed, this slot's own operations stay in flight.  The counts are compile-time constants because every VMEM operation of
// the tile body is unconditional: rows past M are clamped for loads and redirected to a scratch row for stores.
//
// Operand rows: the tile's input rows e are staged through a per-wave 8 KB LDS buffer by LDS-DMA (no registers while in
// flight, re-filled for tile t+1 as soon as tile t's last K-slice has been split); the gathered projections Pd[dst],
// Ps[src] and the residual rows land in two register tiles.  No VMEM instruction is issued inside a GEMM quarter.
//
// Static shape = ShEdge of mgn_x6.inc (4 layers, ReLU, RMSNorm, residual, two gathered adds, fused segment sum), fp32-grade
// (6 terms).  Same arithmetic in the same order as k_mlp_fwd_x6<6, 4, 0, ShEdge>: outputs are bit-identical to it.

#define PP_STAGE_BYTES 8192
#define PP_CST_BYTES (5 * 512)
#define PP_LDS_BYTES (X6_RING * X6_QBYTES + PP_CST_BYTES + 8 * PP_STAGE_BYTES)

// where the stores of rows past M go (never read)
__device__ float g_pp_trash[16 * 128];

#ifdef MGN_TIMELINE
// debug build only (tools/timeline_pp.py): s_memtime stamps of wave 0 (group P) and wave 4 (group Q) of workgroup 0,
// buffered in LDS, dumped when the kernel ends
__device__ unsigned long long g_pp_tl[2][1024];
__device__ int g_pp_tln[2];
#define PP_TL_DECL()                                      \
  __shared__ unsigned long long pp_tl_buf_[2][1024];      \
  int pp_tl_n_ = 0;                                       \
  const bool pp_tl_on_ = blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == 256)
#define PP_STAMP(tag)                                                                                                   \
  do {                                                                                                                  \
    if (pp_tl_on_ && pp_tl_n_ < 1024) pp_tl_buf_[threadIdx.x >> 8][pp_tl_n_++] = (__builtin_readcyclecounter() << 8) | (tag); \
  } while (0)
#define PP_TL_DUMP()                                                                               \
  do {                                                                                             \
    if (pp_tl_on_) {                                                                               \
      for (int i_ = 0; i_ < pp_tl_n_; ++i_) g_pp_tl[threadIdx.x >> 8][i_] = pp_tl_buf_[threadIdx.x >> 8][i_]; \
      g_pp_tln[threadIdx.x >> 8] = pp_tl_n_;                                                       \
    }                                                                                              \
  } while (0)
extern "C" int mgn_debug_pp_timeline(unsigned long long* out, int* n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pp_tl), sizeof(unsigned long long) * 2 * 1024) != hipSuccess) return 1;
  return hipMemcpyFromSymbol(n, HIP_SYMBOL(g_pp_tln), sizeof(int) * 2) != hipSuccess;
}
#else
#define PP_TL_DECL() ((void)0)
#define PP_STAMP(tag) ((void)0)
#define PP_TL_DUMP() ((void)0)
#endif

struct WFrag {
  u32x4 w3[2], w2[2], w1[2][2];
};

// slot boundary: nothing -- memory operations or arithmetic -- is scheduled across it (a free slot's work must not leak
// into the wave's own compute slot, nor the other way round)
__device__ __forceinline__ void pp_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}

// s_waitcnt vmcnt(n) for a compile-time n that is only known after inlining (the counts of a free slot add up in a
// local variable of straight-line code: the switch folds to one case)
__device__ __forceinline__ void pp_vmcnt(int n) {
#define PP_VM(k) \
  case k:        \
    asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); \
    break;
  switch (n) {
    PP_VM(0) PP_VM(1) PP_VM(2) PP_VM(3) PP_VM(4) PP_VM(5) PP_VM(6) PP_VM(7) PP_VM(8) PP_VM(9)
    PP_VM(10) PP_VM(11) PP_VM(12) PP_VM(13) PP_VM(14) PP_VM(15) PP_VM(16) PP_VM(17) PP_VM(18) PP_VM(19)
    PP_VM(20) PP_VM(21) PP_VM(22) PP_VM(23) PP_VM(24) PP_VM(25) PP_VM(26) PP_VM(27) PP_VM(28) PP_VM(29)
    PP_VM(30) PP_VM(31) PP_VM(32) PP_VM(33) PP_VM(34) PP_VM(35) PP_VM(36) PP_VM(37) PP_VM(38) PP_VM(39)
    PP_VM(40) PP_VM(41) PP_VM(42) PP_VM(43) PP_VM(44) PP_VM(45) PP_VM(46) PP_VM(47) PP_VM(48)
    default:
      asm volatile("s_waitcnt vmcnt(48)" ::: "memory");  // more than 48 young operations: over-wait
      break;
  }
#undef PP_VM
}

// first fragments of a quarter (those gemm_q reads before its first MFMA): issued at the END of the free slot before
__device__ __forceinline__ void pp_preload(WFrag& f, lds_char* wl) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    f.w3[q] = *(lds_cu32x4*)(wl + 2 * 8192 + q * 1024);
    f.w2[q] = *(lds_cu32x4*)(wl + 1 * 8192 + q * 1024);
    f.w1[0][q] = *(lds_cu32x4*)(wl + q * 1024);
  }
}
// one quarter: acc[ob] += W[ob-block, K-slice] . x for all 8 output blocks, six terms each, in gemm_q's order
// (w3x1, w2x2, w2x1, w1x3, w1x2, w1x1); nothing but LDS reads and MFMAs.  wl = quarter base + 16 * lane.
__device__ __forceinline__ void pp_gemm_q(f32x4 (&acc)[8], const u32x4 (&x)[3], lds_char* wl, WFrag& f) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bool more = s + 1 < 4;
    const int nb = (2 * (s + 1)) * 1024;
    if (more) {
#pragma unroll
      for (int q = 0; q < 2; ++q) f.w1[(s + 1) & 1][q] = *(lds_cu32x4*)(wl + nb + q * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(f.w3[q], x[0], acc[2 * s + q]);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int q = 0; q < 2; ++q) f.w3[q] = *(lds_cu32x4*)(wl + 2 * 8192 + nb + q * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(f.w2[q], x[1], acc[2 * s + q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(f.w2[q], x[0], acc[2 * s + q]);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int q = 0; q < 2; ++q) f.w2[q] = *(lds_cu32x4*)(wl + 1 * 8192 + nb + q * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(f.w1[s & 1][q], x[2], acc[2 * s + q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(f.w1[s & 1][q], x[1], acc[2 * s + q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[2 * s + q] = MFMA_BF(f.w1[s & 1][q], x[0], acc[2 * s + q]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// blocks 2j, 2j+1 of a T-layout row tile -> the bf16x3 B operand of K-slice j: split_pair_mfma of mgn_x6.inc (the remainders
// come from the matrix pipe: beside a partner that streams MFMAs a VALU instruction costs ~8 cycles of the free slot --
// tools/coissue_probe.hip -- and the VALU split was 44 of them per K-slice)
__device__ __forceinline__ SplitSel pp_split_sel(int, int) { return split_sel<true>(); }
__device__ __forceinline__ void pp_split_pair(const f32x4& b0, const f32x4& b1, u32x4 (&x)[3], const SplitSel& S) {
  split_pair_mfma(b0, b1, x, S);
}

// sum over the 4 lanes that share a row (c, c + 16, c + 32, c + 48) without the LDS crossbar: v_permlane16_swap /
// v_permlane32_swap exchange register halves between two copies (rows 1,3 of one with rows 0,2 of the other; the upper 32
// lanes of one with the lower 32 of the other), so copy + swap + add is a butterfly step.  In asm: the builtin folds the swap
// of two copies of one value to the identity.
__device__ __forceinline__ float pp_rowsum4(float v) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  float s = a + b;
  float a2 = s, b2 = s;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a2), "+v"(b2));
  return a2 + b2;
}

// segmented inclusive scan of TWO feature blocks over the 16 rows of a wave tile (seg_scan16 of mgn_x6.inc, one block
// at a time: the scan is independent per feature, so the aggregation can be cut into the same pieces as the rest of the
// epilogue).  same[st] = 1 where the row 2^st above has the same key: computed once per tile (pp_seg_same).
__device__ __forceinline__ void pp_seg_same(float (&same)[4], int key) {
  const int k1 = __builtin_amdgcn_update_dpp(-2, key, 0x111, 0xf, 0xf, false);
  const int k2 = __builtin_amdgcn_update_dpp(-2, key, 0x112, 0xf, 0xf, false);
  const int k4 = __builtin_amdgcn_update_dpp(-2, key, 0x114, 0xf, 0xf, false);
  const int k8 = __builtin_amdgcn_update_dpp(-2, key, 0x118, 0xf, 0xf, false);
  same[0] = (k1 == key) ? 1.f : 0.f;
  same[1] = (k2 == key) ? 1.f : 0.f;
  same[2] = (k4 == key) ? 1.f : 0.f;
  same[3] = (k8 == key) ? 1.f : 0.f;
}
__device__ __forceinline__ void pp_seg_scan_blk(f32x4& u0, const float (&same)[4]) {
#define PP_FMAC_DPP4(N, V, S)                                                                          \
  {                                                                                                    \
    float v0 = V[0], v1 = V[1], v2 = V[2], v3 = V[3];                                                   \
    asm volatile("s_nop 1\n\t"                                                                          \
                 "v_fmac_f32_dpp %0, %0, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
                 "v_fmac_f32_dpp %1, %1, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
                 "v_fmac_f32_dpp %2, %2, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
                 "v_fmac_f32_dpp %3, %3, %4 row_shr:" #N " row_mask:0xf bank_mask:0xf bound_ctrl:1"     \
                 : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3)                                               \
                 : "v"(S));                                                                             \
    V[0] = v0, V[1] = v1, V[2] = v2, V[3] = v3;                                                         \
  }
  PP_FMAC_DPP4(1, u0, same[0])
  PP_FMAC_DPP4(2, u0, same[1])
  PP_FMAC_DPP4(4, u0, same[2])
  PP_FMAC_DPP4(8, u0, same[3])
#undef PP_FMAC_DPP4
}

// (Tried: loads the compiler does not track, ordered by the slots' own drains as in mgn_x6.inc's static shapes -- no faster,
// and wrong here: the tile loop is rolled, the landing registers are loop-carried.)

// TRAIN: every save of the training-mode launch (saveH[0..2], saveM[0..2], saveU, saveR) is written; otherwise none.
// Rows past M: loads re-read row M - 1, so such a lane computes row M - 1's results bit for bit and STORES them to row
// M - 1 again (identical bytes; needs outputs that alias no input: checked by the launcher).  Only the run-end stores of
// the segmented scan need a scratch row.
//
// Free-slot schedule of a tile (F(u,q) = the free slot after quarter q of unit u; every slot also splits the K-slice the
// next quarter consumes -- ReLU applied to that block pair on the way; at most ~4 row-sized memory instructions per slot
// and wave: a CU moves ~10-13 bytes per cycle, a burst of 8 KB per wave stalls the issuing waves for thousands of cycles
// and the matrix pipe with them).  Beside a partner that streams MFMAs a wave issues one VALU instruction per ~8 cycles
// (tools/coissue_probe.hip), so a slot of ~850 cycles holds ~100 of them: the work is cut to that.
//   F(3,3)  z complete: row norms, where the run ends of the aggregation go; z -> hb; the next tile opens (rows 0,1 from
//           the stage)
//   F(0,j)  epilogue pair j of the PREVIOUS tile (y, out, [U], segmented scan of y, run-end stores), then the residual
//           registers er[2j], er[2j+1] are refilled with the new tile's rows; F(0,0) adds Pd[dst] and sends for Ps[src]
//   F(0,3)  also + Ps[src]; the pre-activations move to hb; the stage is free: the next tile's rows start to arrive
//   F(1,q)  [H1 saves]  stage pieces, the next tile's gather rows;   F(2,q) [H2 saves], the next tile's Pd[dst] rows
//   F(3,q)  [H3 saves]
//   the bias of the next unit is read from LDS one slot ahead (bq).
template <bool TRAIN>
__global__ void __launch_bounds__(512, 2) k_edge_fwd_pp(const mgn_mlp_fwd_args a) {
  constexpr int HB = 8, H = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* ring = (lds_char*)smem;
  lds_char* cst = ring + X6_RING * X6_QBYTES;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wv >> 2, wq = wv & 3;  // group P (0) / Q (1); wave of the group
  const int c = lane & 15, g = lane >> 4;
  const unsigned lane16 = 16u * lane;
  lds_char* stage = cst + PP_CST_BYTES + wv * PP_STAGE_BYTES;
  const unsigned ring0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring));
  const unsigned stage0 = __builtin_amdgcn_readfirstlane(lds_addr_of(stage));
  PP_TL_DECL();
  const long M = a.M;
  const long ndt = (M + 127) / 128;  // 128-row workgroup tiles: rows [128 dt + 64 grp + 16 wq, +16) belong to this wave
  if ((long)blockIdx.x >= ndt) return;
  const long my_iters = (ndt - blockIdx.x + gridDim.x - 1) / gridDim.x;
  const long K = my_iters * 16;  // quarters of this workgroup's weight stream
  const char* U0 = (const char*)a.wpk[0];  // the four units back to back (checked by the launcher)
  const float* e_rows = a.src[0];
  const float *Pd = a.add_src[0], *Ps = a.add_src[1];
  const int32_t *dsti = a.add_idx[0], *srci = a.add_idx[1];

  // Row tensors of M x 128 floats are addressed as (uniform base) + (32-bit byte offset of this lane's 16 bytes in block 0)
  // + 64 * block: ONE offset register serves every tensor of the tile (the launcher keeps M * 512 below 4 GB)
  auto at = [](const float* base, unsigned off, int ib) -> float* { return (float*)((char*)base + (size_t)off + 64 * ib); };

  // ---- prologue: quarters 0..2 (3 pieces per wave each), constants, the first tile's operands
#pragma unroll
  for (int k = 0; k < X6_RING; ++k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int off = k * X6_QBYTES + (wv * 3 + i) * 1024;
      glds16c((const char*)uniform_ptr((const float*)(U0 + off)), lane16, ring0 + off);
    }
  }
  for (int i = threadIdx.x; i < 5 * H; i += 512) {
    const int l = i >> 7, jx = i & 127;
    const float* bp = (l == 4) ? a.scale : pick4(a.b[0], a.b[1], a.b[2], a.b[3], l);
    ((__attribute__((address_space(3))) float*)cst)[i] = (bp != nullptr) ? bp[jx] : 0.f;
  }
  auto lds_bias = [&](f32x4 (&v)[HB], int l) {
#pragma unroll
    for (int ib = 0; ib < HB; ++ib) v[ib] = *(lds_cf32x4*)(cst + l * 512 + 64 * ib + 16 * g);
  };
  auto tile_m0 = [&](long it) -> long { return ((long)blockIdx.x + it * gridDim.x) * 128 + grp * 64 + wq * 16; };
  // the tile's input rows -> the wave's LDS stage: piece ib = bytes [64 ib, +64) of each of the 16 rows, lane (c, g) owns
  // 16 of them (T-layout block ib); two pieces per call
  auto stage_issue2 = [&](long m0_, int ib0, int& nv) {
    const long lim = (M >= 16) ? M - 16 : 0;
    const long mb = (m0_ < lim) ? m0_ : lim;  // wave-uniform base row (offsets below are >= 0)
    long row = m0_ + c;
    row = (row < M) ? row : M - 1;
    const unsigned voff = (unsigned)((row - mb) * 512 + 16 * g);
    const float* sb = uniform_ptr(e_rows + mb * H);
    glds16(sb + 16 * ib0, voff, stage0 + ib0 * 1024);
    glds16(sb + 16 * (ib0 + 1), voff, stage0 + (ib0 + 1) * 1024);
    nv += 2;
  };
  auto stage_blk = [&](int ib) -> f32x4 { return *(lds_cf32x4*)(stage + ib * 1024 + lane16); };
  auto row_off = [&](long m0_) -> unsigned {  // byte offset of this lane's piece of block 0 of its (clamped) row
    const long m = m0_ + c;
    return (unsigned)(((m < M) ? m : M - 1) * 512 + 16 * g);
  };

  long m0 = tile_m0(0);       // current tile: first row of the wave tile
  unsigned ro = row_off(m0);  // ... and this lane's row offset
  int rd, rs, rdn = 0, rsn = 0;  // gather rows (dst, src) of the current / next tile
  int nbk = 0;                   // keys of the rows either side of the current wave tile (lanes c < 8 / c >= 8)
  // previous tile (its epilogue runs block by block under the current tile's first nine quarters): row offset, where this
  // lane's run-end rows of the aggregation go (the scratch row unless the row ends a run), the scan's same-key masks, the
  // row's sum of squares -> 1 / (rms + eps).  Before the first tile (`first`) the epilogue slots LOAD where they would store:
  // the same instruction counts, nothing written; the run-end store of lane 0 goes to the scratch row.
  bool first = true;
  unsigned pro = ro;
  float* pseg = g_pp_trash + c * H + 4 * g;
  bool pact = (lane == 0);  // lanes that store in the segment step: run ends, and lane 0 so that the instruction always issues
  float psame[4] = {0.f, 0.f, 0.f, 0.f};
  float pinv = 0.f, pss = 0.f;
  {
    const long m = m0 + c;
    const long mm = (m < M) ? m : M - 1;
    rd = dsti[mm];
    rs = srci[mm];
  }
  // The residual e + y needs the tile's input rows once more, nine quarters after their last K-slice was split.  Inference
  // mode keeps them in registers (er, refilled from the stage block by block as the epilogue consumes the old ones); the
  // training-mode instance has no 32 registers left (its saves need the activations alive longer) and reads the pieces again,
  // one block per epilogue slot, one slot ahead (enext): L2 / Infinity-Cache hits, 8 more memory instructions per tile.
  constexpr bool KEEP_E = !TRAIN;
  f32x4 acc[HB], hb[HB], er[KEEP_E ? HB : 1], pr[HB], zb[HB];
  f32x4 enext = {0.f, 0.f, 0.f, 0.f};
  const SplitSel sel = pp_split_sel(c, g);
  u32x4 xs[3];
  WFrag wf;
  {
    int nv = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) stage_issue2(m0, 2 * j, nv);
  }
#pragma unroll
  for (int kb = 0; kb < HB; ++kb) pr[kb] = ld4(Pd + (long)rd * H + 4 * g + 16 * kb);
#pragma unroll
  for (int kb = 0; kb < HB; ++kb) hb[kb] = ld4(Ps + (long)rs * H + 4 * g + 16 * kb);
#pragma unroll
  for (int kb = 0; kb < (KEEP_E ? HB : 1); ++kb) er[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < HB; ++kb) zb[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  dma_drain();
  __syncthreads();
  lds_bias(acc, 0);
  pp_split_pair(stage_blk(0), stage_blk(1), xs, sel);
  pp_preload(wf, ring + lane16);

  long qi = 0;    // quarter of the stream this wave computes next
  int cslot = 0;  // its ring slot
  if (grp) pp_barrier();  // Q lags P by one slot

  // the closing part of a free slot: first fragments of the next quarter, the ring refill (Q), the counted drain
  auto close_slot = [&](int nv) {
    // what the next quarter consumes is pinned HERE (hipcc otherwise sinks the split and the accumulator updates towards
    // their use, behind the drain below and partly behind the barrier)
    asm volatile("" : "+v"(xs[0]), "+v"(xs[1]), "+v"(xs[2]));
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]));
    __builtin_amdgcn_sched_barrier(0);
    PP_STAMP(4);
    const int nslot = (cslot == X6_RING - 1) ? 0 : cslot + 1;
    pp_preload(wf, ring + nslot * X6_QBYTES + lane16);
    if (grp) {  // refill the ring slot this group has just finished reading: quarter qi + 3
      DmaQ job;
      const long qn = qi + 3;
      job.on = qn < K;
      job.su = (const char*)uniform_ptr((const float*)(U0 + (qn & 15) * X6_QBYTES + wq * 6144));
      job.lds = ring0 + cslot * X6_QBYTES + wq * 6144;
      dmaq_issue2<0>(job, lane16);
      dmaq_issue2<1>(job, lane16);
      dmaq_issue2<2>(job, lane16);
      if (job.on)
        pp_vmcnt(nv + 6);
      else
        pp_vmcnt(nv);
    } else {
      pp_vmcnt(nv);
    }
    ++qi;
    cslot = nslot;
  };
  // One step of the stream: my compute slot, then my free slot.  `work(nv)` is the free slot's piece of the tile's
  // non-GEMM work; it adds the VMEM operations it issues (all unconditional) to nv.
  auto step = [&](auto work) {
    PP_STAMP(0);
    pp_barrier();
    PP_STAMP(1);
    __builtin_amdgcn_s_setprio(2);  // wave priority: 2 inside a GEMM quarter, 0 inside a free slot
    pp_gemm_q(acc, xs, ring + cslot * X6_QBYTES + lane16, wf);
    __builtin_amdgcn_s_setprio(0);
    PP_STAMP(2);
    pp_barrier();
    PP_STAMP(3);
    int nv = 0;
    work(nv);
    close_slot(nv);
  };

  // ---- pieces of the non-GEMM work
  // unit boundary: the pre-activations leave the accumulators (ReLU is applied pair by pair when they are split) and the
  // accumulators restart from the next layer's bias -- read into the registers the previous activations have left (acc and
  // hb trade places: no copies; issued first in the slot, so the LDS latency passes under the slot's arithmetic)
  auto boundary = [&](int l) {
#pragma unroll
    for (int ib = 0; ib < HB; ++ib) hb[ib] = acc[ib];
    lds_bias(acc, l);
  };
  auto relu_split = [&](int j) {
#pragma unroll
    for (int ib = 2 * j; ib < 2 * j + 2; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = hb[ib][r];
        asm("v_max_f32 %0, 0, %0" : "+v"(v));  // one instruction (fmaxf also quiets NaNs: two)
        hb[ib][r] = v;
      }
    pp_split_pair(hb[2 * j], hb[2 * j + 1], xs, sel);
  };
  // saves of layer l's activation (training mode), block pair j: the rows, and -- with the last pair -- their sign bits
  u32 mbits = 0;
  auto save_h2 = [&](int l, int j, int& nv) {
    if constexpr (TRAIN) {
      const float* sh = pick3(a.saveH[0], a.saveH[1], a.saveH[2], l);
      st4_stream(at(sh, ro, 2 * j), hb[2 * j]);
      st4_stream(at(sh, ro, 2 * j + 1), hb[2 * j + 1]);
      nv += 2;
      if (j == 0) mbits = 0;
#pragma unroll
      for (int ib = 2 * j; ib < 2 * j + 2; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) mbits |= (hb[ib][r] > 0.f) ? (1u << (4 * ib + r)) : 0u;
      if (j == 3) {  // row m, word g: byte 16 m + 4 g
        *(__attribute__((address_space(1))) u32*)((char*)pick3(a.saveM[0], a.saveM[1], a.saveM[2], l) + (size_t)(((ro >> 9) << 4) + 4 * g)) = mbits;
        nv += 1;
      }
    }
  };
  // epilogue of the previous tile (z in zb, its input rows in er), block ib: u = z / (rms + eps), y = scale * u,
  // out = e + y, the fused aggregation of y (segmented scan over the wave tile's 16 rows; run-end lanes store to seg_out /
  // seg_part); then the residual registers take the NEW tile's rows (still in the stage)
  auto epi_blk = [&](int ib, int& nv) {
    const f32x4 sc4 = *(lds_cf32x4*)(cst + 4 * 512 + 64 * ib + 16 * g);
    f32x4 u, y, o;
    const f32x4 e4 = KEEP_E ? er[ib] : enext;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u[r] = zb[ib][r] * pinv;
      y[r] = sc4[r] * u[r];
      o[r] = e4[r] + y[r];
    }
    if constexpr (!KEEP_E) {  // the next block's residual piece (read again from memory: see KEEP_E)
      enext = ld4(at(a.resid, pro, (ib + 1) & 7));
      nv += 1;
    }
    if (first) {  // no previous tile yet: the same number of memory instructions (the counts are static), as loads
      f32x4 t0 = ld4(at(a.out, pro, ib));
      asm volatile("" ::"v"(t0));
      if constexpr (TRAIN) {
        f32x4 t1 = ld4(at(a.saveU, pro, ib));
        asm volatile("" ::"v"(t1));
      }
    } else {
      if constexpr (TRAIN) st4_stream(at(a.saveU, pro, ib), u);
      st4(at(a.out, pro, ib), o);
    }
    nv += TRAIN ? 2 : 1;
    pp_seg_scan_blk(y, psame);
    if (pact) st4(pseg + 16 * ib, y);
    nv += 1;
    if constexpr (KEEP_E) er[ib] = stage_blk(ib);
  };
  // the new tile's rows 2j, 2j+1 from the stage -> the next quarter's operand
  auto open_pair = [&](int j) { pp_split_pair(stage_blk(2 * j), stage_blk(2 * j + 1), xs, sel); };
  auto norms = [&](int& nv) {  // the previous tile's row norms (reference epsilon placement)
    const float rms = sqrtf(pss) / sqrtf((float)H);
    pinv = 1.0f / (rms + a.eps);
    if constexpr (!KEEP_E) {
      enext = ld4(at(a.resid, pro, 0));
      nv += 1;
    }
    if constexpr (TRAIN) {  // row m: byte 4 m = pro / 128 (g == 0 lanes exact; the others write the same word)
      float* rp = (float*)((char*)a.saveR + (size_t)((pro >> 9) << 2));
      if (first) {
        float t0 = ld1(rp);
        asm volatile("" ::"v"(t0));
      } else {
        st1(rp, rms);
      }
      nv += 1;
    }
  };
  auto ld_pd = [&](int ib, int& nv) {  // the next tile's Pd[dst] rows, one block per slot
    pr[ib] = ld4(Pd + (long)rdn * H + 4 * g + 16 * ib);
    nv += 1;
  };
  auto ld_ps2 = [&](int j, int& nv) {  // the next tile's Ps[src] rows land in the activation registers H3 has just left
    hb[2 * j] = ld4(Ps + (long)rsn * H + 4 * g + 16 * (2 * j));
    hb[2 * j + 1] = ld4(Ps + (long)rsn * H + 4 * g + 16 * (2 * j + 1));
    nv += 2;
  };

  for (long it = 0; it <= my_iters; ++it) {
    if (it == my_iters) {
      // ---- tail: the last tile's epilogue (P first leaves the slot it owes Q)
      if (!grp) pp_barrier();
      int nv = 0;
      norms(nv);
#pragma unroll
      for (int ib = 0; ib < HB; ++ib) epi_blk(ib, nv);
      PP_TL_DUMP();
      break;
    }
    const long m0n = tile_m0(it + 1);
    // ================= unit 0: W_e . e  (operand from the LDS stage) =================
    step([&](int& nv) {  // s0 = F(0,0): + Pd[dst]; the next tile's gather rows
      norms(nv);
      open_pair(1);
#pragma unroll
      for (int ib = 0; ib < HB; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ib][r] += pr[ib][r];
      const long m = m0n + c;
      const long mmn = (m < M) ? m : M - 1;
      rdn = dsti[mmn];
      rsn = srci[mmn];
      nv += 2;
    });
    step([&](int& nv) {  // s1
      epi_blk(0, nv);
      open_pair(2);
    });
    step([&](int& nv) {  // s2
      epi_blk(1, nv);
      open_pair(3);
    });
    step([&](int& nv) {  // s3 = F(0,3): z0 = W_e e + b0 + Pd[dst] + Ps[src] -> hb (in place: Ps landed there); accumulators restart from b1
      epi_blk(2, nv);
#pragma unroll
      for (int ib = 0; ib < HB; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) hb[ib][r] = acc[ib][r] + hb[ib][r];
      lds_bias(acc, 1);
      relu_split(0);
      save_h2(0, 0, nv);
    });
    // ================= unit 1 =================
    step([&](int& nv) {  // s4
      epi_blk(3, nv);
      relu_split(1);
      save_h2(0, 1, nv);
      ld_pd(0, nv);
    });
    step([&](int& nv) {  // s5
      epi_blk(4, nv);
      relu_split(2);
      save_h2(0, 2, nv);
      ld_pd(1, nv);
    });
    step([&](int& nv) {  // s6
      epi_blk(5, nv);
      relu_split(3);
      save_h2(0, 3, nv);
      ld_pd(2, nv);
    });
    step([&](int& nv) {  // s7 = F(1,3)
      boundary(2);
      epi_blk(6, nv);
      relu_split(0);
      save_h2(1, 0, nv);
      ld_pd(3, nv);
    });
    // ================= unit 2 =================
    step([&](int& nv) {  // s8
      epi_blk(7, nv);
      relu_split(1);
      save_h2(1, 1, nv);
      ld_pd(4, nv);
    });
    step([&](int& nv) {  // s9: every block of the stage has been taken over: the next tile's rows start to arrive
      relu_split(2);
      save_h2(1, 2, nv);
      ld_pd(5, nv);
      stage_issue2(m0n, 0, nv);
    });
    step([&](int& nv) {  // s10: the keys of the rows either side of this wave tile
      relu_split(3);
      save_h2(1, 3, nv);
      ld_pd(6, nv);
      stage_issue2(m0n, 2, nv);
      long rk = (c < 8) ? m0 - 1 : m0 + 16;
      rk = (rk < 0) ? 0 : rk;
      rk = (rk < M) ? rk : M - 1;
      nbk = a.seg_key[rk];
      nv += 1;
    });
    step([&](int& nv) {  // s11 = F(2,3)
      boundary(3);
      relu_split(0);
      save_h2(2, 0, nv);
      ld_pd(7, nv);
      stage_issue2(m0n, 4, nv);
      ld_ps2(0, nv);  // H3 blocks 0, 1 are split and saved: the next tile's Ps[src] rows may land there
    });
    // ================= unit 3 =================
    step([&](int& nv) {  // s12
      relu_split(1);
      save_h2(2, 1, nv);
      stage_issue2(m0n, 6, nv);
      ld_ps2(1, nv);
    });
    step([&](int& nv) {  // s13: where this tile's run ends of the aggregation will go
      relu_split(2);
      save_h2(2, 2, nv);
      ld_ps2(2, nv);
      const int key = (m0 + c < M) ? rd : -1;
      const int kprev = (m0 > 0) ? __builtin_amdgcn_readlane(nbk, 0) : -1;
      const int knxt = (m0 + 16 < M) ? __builtin_amdgcn_readlane(nbk, 15) : -1;
      const int knext = __builtin_amdgcn_update_dpp(-3, key, 0x101, 0xf, 0xf, false);  // row_shl:1, lane 15 keeps -3
      const int key0 = __builtin_amdgcn_readfirstlane(key);
      const bool run_end = key >= 0 && knext != key;
      const bool before = (key == key0) && (kprev == key0);
      const bool inside = !before && !(knext == -3 && knxt == key);
      float* dst = g_pp_trash + c * H;
      if (run_end) dst = inside ? a.seg_out + (long)key * H : a.seg_part + ((m0 >> 4) * 2 + (before ? 0 : 1)) * H;
      pseg = dst + 4 * g;
      pact = run_end || lane == 0;
      pp_seg_same(psame, key);
    });
    step([&](int& nv) {  // s14
      relu_split(3);
      save_h2(2, 3, nv);
      ld_ps2(3, nv);
    });
    step([&](int& nv) {  // s15 = F(3,3): z is complete: sum of squares of every row; z -> zb; the next tile opens
      float ss = 0.f;
#pragma unroll
      for (int ib = 0; ib < HB; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss = fmaf(acc[ib][r], acc[ib][r], ss);
      pss = pp_rowsum4(ss);
      // z -> zb by 32 real copies: acc and zb would otherwise trade places once per tile, and a loop body must leave every
      // array where it found it (the alternative is two tiles per loop iteration: twice the instruction footprint)
#pragma unroll
      for (int ib = 0; ib < HB; ++ib) zb[ib] = acc[ib];
      lds_bias(acc, 0);
      pro = ro;
      first = false;
      m0 = m0n;
      ro = row_off(m0);
      rd = rdn, rs = rsn;
      open_pair(0);
    });
  }
}
