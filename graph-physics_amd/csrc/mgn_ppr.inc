// "Register-resident weights" generation of the split-bf16 edge update [r6] (included by mgn_kernels.hip after mgn_pp.inc).
//
// Why.  The x6 chain kernels stream every 128x128 unit through a 72 KB LDS ring, quarter by quarter, once per 64-row tile: per
// 48 MFMAs a wave issues 24 ds_read_b128 of weight fragments, a counted DMA drain and a barrier, and the SAME wave also loads, splits,
// masks and stores its rows (DESIGN 4.2: 211 us per training-mode launch of which 82 us are the matrix work).  Here the weights never
// move after the prologue and the two kinds of work belong to different waves of a SIMD:
//
//   * ONE 512-thread workgroup per CU.  Wave (h, w), h = wave >> 2, w = wave & 3, owns output blocks {2w, 2w+1} (32 of the 128
//     features) of the units {2h, 2h+1}: 2 units x 2 blocks x 4 K-slices x 3 bf16 pieces = 48 x 16 bytes = 192 registers, loaded
//     once from the mgn_wpack image.  Waves h = 0 run the chain's first half (W_e . e, layer 1), waves h = 1 the second (layers 2, 3),
//     one group of R = 2 sixteen-row tiles behind.
//   * The B operands (the rows' bf16x3 pieces, 12 KB per tile) live in LDS: a wave reads all of them (12 ds_read_b128 per tile and
//     unit against 48 MFMAs: a quarter of the x6 kernels' fragment reads) and, after its own 32 features are done, writes K-slice w
//     of the NEXT unit's operand (3 ds_write_b128): two 16-wide blocks packed to bf16 are exactly one K-slice (mgn_x6.inc, T layout).
//   * Time is cut into slots of two phases by s_barrier.  Phase A: waves h = 0 multiply (nothing but LDS reads and MFMAs), waves
//     h = 1 do the non-matrix work of the unit they finished in the previous slot (ReLU, saves, mask, matrix-pipe split; or the tile
//     epilogue: RMSNorm, residual, stores, fused aggregation).  Phase B: the roles swap.  Each SIMD hosts one wave of either half, so
//     in every phase its matrix pipe is fed by one wave while the other issues the vector / memory instructions
//     (tools/ppr_probe.hip: 17.8 cycles per MFMA for the bare phases, 21.5 with the non-matrix work beside them).
//   * Operand rows arrive by LDS-DMA in whole 512-byte rows (two rows per instruction: 17 texture-addresser cycles against 64 for
//     a T-layout load, profiles/r04_ta_probe.txt), issued by the h = 0 waves one slot ahead: the tile's e rows (contiguous) and the
//     gathered Pd[dst] / Ps[src] rows.  16-byte chunk ch of tile row c sits at slot ch ^ c of the row's 32: a T-layout
//     ds_read_b128 (lane (c, g), block ib -> chunk 4 ib + g) is conflict-free.
//
// Static shape = ShEdge of mgn_x6.inc (4 layers, ReLU, RMSNorm, residual, two gathered adds, fused segment sum), fp32-grade
// (6 terms).  The MFMA terms run in gemm_q's order on the same packed weights, so H1..H3, the masks and z are bit-identical to
// k_mlp_fwd_x6<6, 4, 0, ShEdge>; the row norm adds its 128 squares in another order (4 partial sums of 32), so u, out and the
// aggregate agree to rounding (~1e-7), not bit for bit.  Rows past M are computed as copies of row M - 1 and stored there again
// (identical bytes; outputs must alias no input: checked by the launcher), their aggregation key is -1.
//
// Slots (g = group of this workgroup, two slots per group and half):
//     slot      2g            2g+1            2g+2           2g+3            2g+4
//     h = 0   A: GEMM u0    A: GEMM u1     (group g+1)
//             B: post u0    B: post u1 -> Qin, split e(g+1) -> P
//     h = 1                                A: ...          A: post u2      A: epilogue(g)
//                                          B: GEMM u2      B: GEMM u3, row sums of squares
// LDS: P (operand of h = 0), Qin (unit 2, written by h = 0), Qown (unit 3), Pd / Ps rows, a ring of three groups of e rows (the rows
// are the operand of the first unit AND, eleven phases later, the residual of the epilogue), constants, partial square sums, selectors.

#define PPR_R 2
// Saves of the training-mode launches (H1..H3, u; the backward chain's dZ rows) as NON-TEMPORAL stores: a wave of these kernels writes
// the two 64-byte halves of a 128-byte line in consecutive instructions, so nothing is lost by not merging them in L2 (the x6 kernels
// paid +12 % write traffic for it), and the write-back cache no longer sits between a store and its acknowledgement: the counted
// waits for the LDS-DMA rows stop queueing behind the stores of the boundary before (186 -> 149-161 us for the training-mode forward,
// alternating in one GPU call).  So is the backward chain's dE.  e' (`out`, re-read by the next launch) stays a plain store (st4).
#define PPR_TILE_PIECES (12 * 1024)
#define PPR_IMG (PPR_R * PPR_TILE_PIECES)
#define PPR_OFF_P 0
#define PPR_OFF_QIN PPR_IMG
#define PPR_OFF_QOWN (2 * PPR_IMG)
#define PPR_OFF_G (3 * PPR_IMG)                      /* Pd[dst] | Ps[src] rows of a group */
#define PPR_OFF_E (PPR_OFF_G + PPR_R * 16384)       /* ring of THREE groups of e rows: a group's rows are split in phase 4g - 1 and are */
#define PPR_E_SLOT (PPR_R * 8192)                   /* the residual of its epilogue in phase 4g + 8 -- no second fetch (92 MB per launch) */
#define PPR_OFF_CST (PPR_OFF_E + 3 * PPR_E_SLOT)
#define PPR_OFF_SSQ (PPR_OFF_CST + 5 * 512)
#define PPR_OFF_SEL (PPR_OFF_SSQ + PPR_R * 256)  /* the two selector operands of the matrix-pipe split, 1 KB each */
#define PPR_LDS_BYTES (PPR_OFF_SEL + 2048)

#ifdef MGN_TIMELINE
// debug build only (tools/timeline_ppr.py): s_memtime stamps of wave 0 (h = 0) and wave 4 (h = 1) of workgroup 0
__device__ unsigned long long g_ppr_tl[2][160];   // (2.5 KB of LDS beside the kernels' 150-157 KB: the first groups of the workgroup)
__device__ int g_ppr_tln[2];
#define PPR_TL_DECL()                                       \
  __shared__ unsigned long long ppr_tl_buf_[2][160];        \
  int ppr_tl_n_ = 0;                                        \
  const bool ppr_tl_on_ = blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == 256)
#define PPR_STAMP(tag)                                                                                                          \
  do {                                                                                                                          \
    if (ppr_tl_on_ && ppr_tl_n_ < 160) ppr_tl_buf_[threadIdx.x >> 8][ppr_tl_n_++] = (__builtin_readcyclecounter() << 8) | (tag); \
  } while (0)
#define PPR_TL_DUMP()                                                                                          \
  do {                                                                                                         \
    if (ppr_tl_on_) {                                                                                          \
      for (int i_ = 0; i_ < ppr_tl_n_; ++i_) g_ppr_tl[threadIdx.x >> 8][i_] = ppr_tl_buf_[threadIdx.x >> 8][i_]; \
      g_ppr_tln[threadIdx.x >> 8] = ppr_tl_n_;                                                                 \
    }                                                                                                          \
  } while (0)
extern "C" int mgn_debug_ppr_timeline(unsigned long long* out, int* n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ppr_tl), sizeof(unsigned long long) * 2 * 160) != hipSuccess) return 1;
  return hipMemcpyFromSymbol(n, HIP_SYMBOL(g_ppr_tln), sizeof(int) * 2) != hipSuccess;
}
#else
#define PPR_TL_DECL() ((void)0)
#define PPR_STAMP(tag) ((void)0)
#define PPR_TL_DUMP() ((void)0)
#endif

__device__ __forceinline__ void ppr_st4_nt(float* p, f32x4 v) { __builtin_nontemporal_store(v, (g_f32x4*)p); }
// phase boundary: LDS writes of this wave are done, nothing is scheduled across it
__device__ __forceinline__ void ppr_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}

// make a per-lane value opaque: what is derived from it inside the group loop is re-derived there (one or two instructions)
// instead of being hoisted into its own loop-long register -- the kernel keeps 192 registers of weights, every loop-invariant
// address the compiler forms costs a spill
__device__ __forceinline__ unsigned ppr_opaque(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ lds_char* ppr_lds(unsigned addr) { return (lds_char*)(size_t)addr; }

// Two LDS-DMAs of 1 KB into consecutive LDS blocks with ONE save / restore of M0 (see glds16 of mgn_kernels.hip): lane L fetches
// 16 bytes at sbase + voff0(L) into lds_addr + 16 L and 16 bytes at sbase + voff1(L) into lds_addr + 1024 + 16 L.  The leading
// s_nop covers a VALU-written SGPR operand (v_readfirstlane): the compiler does not look into the statement.
__device__ __forceinline__ void glds16x2(const float* sbase, unsigned voff0, unsigned voff1, unsigned lds_addr) {
  unsigned keep;
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %3\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %3\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff0), "v"(voff1), "s"(sbase), "s"(lds_addr)
      : "memory", "scc");
}

template <bool TRAIN, bool XCD>
__global__ void __launch_bounds__(512, 2) k_edge_fwd_ppr(const mgn_mlp_fwd_args a) {
  constexpr int H = 128, R = PPR_R;
  // GH1: the gathered rows Pd[dst] / Ps[src] of a group are asked for by the SECOND half's waves, in their first boundary phase -- one phase
  // earlier than the first half could (the buffer is free as soon as the first half's unit-0 boundary has read it), and waited for at the
  // end of their epilogue phase: 2.5 phases to land instead of 1.5, and the first half's heaviest boundary loses four LDS-DMA pairs
  // (measured in situ, alternating: inference 132-134 against 134-140 us with the gathers asked for by the second half, training mode
  // 201-206 against 193-197 us -- its extra scalar state spills two weight fragments -- so the training-mode instance keeps them in the first half)
  constexpr bool GH1 = !TRAIN;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* sm = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = wave >> 2, w = wave & 3;
  const int c = lane & 15, g = lane >> 4;
  const unsigned sm0 = __builtin_amdgcn_readfirstlane(lds_addr_of(sm));
  PPR_TL_DECL();
  const int M = (int)a.M;               // (the launcher keeps M * 512 below 4 GB)
  const int T = (M + 15) / 16;          // 16-row tiles
  const int NG = (T + R - 1) / R;       // groups of R tiles
  const int G = gridDim.x;
  const int per = (NG + G - 1) / G;
  // XCD-aware hand-out: workgroup b runs on XCD b % 8 (observed, for speed only); XCD x walks one contiguous eighth of the groups,
  // so the node rows its workgroups gather (dst-sorted edges: neighbouring rows) stay in that XCD's L2
  int cb = blockIdx.x;
  if (XCD && (G & 7) == 0) cb = (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3);
  const int g0 = cb * per;
  const int g1 = (g0 + per < NG) ? g0 + per : NG;
  if (g0 >= g1) return;
  const int ng = g1 - g0;

  // ---- the wave's weights: units 2h, 2h+1 (back to back with unit 0: checked by the launcher), blocks 2w, 2w+1
  u32x4 W[2][3][2][4];  // [unit of the half][piece][block][K-slice]
  {
    const char* wb = (const char*)a.wpk[0] + (size_t)(2 * h) * MGN_WPACK_BYTES + (size_t)(2 * w) * 1024 + 16u * lane;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            W[u][p][q][j] = *(const __attribute__((address_space(1))) u32x4*)(wb + (size_t)u * MGN_WPACK_BYTES + j * X6_QBYTES + p * 8192 + q * 1024);
  }
  for (int i = threadIdx.x; i < 5 * H; i += 512) {
    const int l = i >> 7, jx = i & 127;
    const float* bp = (l == 4) ? a.scale : pick4(a.b[0], a.b[1], a.b[2], a.b[3], l);
    ((__attribute__((address_space(3))) float*)(sm + PPR_OFF_CST))[i] = (bp != nullptr) ? bp[jx] : 0.f;
  }
  if (wave == 0) {  // the selector operands of the matrix-pipe split (mgn_x6.inc split_sel): read back in every non-matrix phase
    const SplitSel S0 = split_sel<true>();
    *(__attribute__((address_space(3))) u32x4*)(sm + PPR_OFF_SEL + 16 * lane) = S0.s0;
    *(__attribute__((address_space(3))) u32x4*)(sm + PPR_OFF_SEL + 1024 + 16 * lane) = S0.s1;
  }
  // ---- the per-lane LDS addresses of the whole kernel: five registers, everything else is an immediate offset from one of them
  //   pA / pB : piece image of the half's first / second unit + 16 lane   (h = 0: P, P; h = 1: Qin, Qown)
  //   lq[q]   : this lane's 16 bytes of block 2w + q in a landed 16-row tile at PPR_OFF_G (row c at byte 512 c, chunk ch at slot ch ^ c);
  //             the e rows of group gi: + eoff(gi) (the ring slot: a scalar added per use)
  //   cq      : constants: bias row 2h, block 2w, lane group g
  const unsigned pA = ppr_opaque(sm0 + (h ? PPR_OFF_QIN : PPR_OFF_P) + 16u * lane);
  const unsigned pB = ppr_opaque(sm0 + (h ? PPR_OFF_QOWN : PPR_OFF_P) + 16u * lane);
  const unsigned lq0 = ppr_opaque(sm0 + PPR_OFF_G + c * 512 + 16 * ((4 * (2 * w) + g) ^ c));
  const unsigned lq1 = ppr_opaque(sm0 + PPR_OFF_G + c * 512 + 16 * ((4 * (2 * w + 1) + g) ^ c));
  auto eoff = [&](int gi) -> unsigned { return (unsigned)(PPR_OFF_E - PPR_OFF_G) + (unsigned)(gi % 3) * PPR_E_SLOT; };
  const unsigned cq = ppr_opaque(sm0 + PPR_OFF_CST + (2 * h) * 512 + 64 * (2 * w) + 16 * g);
  f32x4 acc[R][2];

  // first row of tile r of group gi (local index); this lane's (clamped) row and its byte offset in an M x 128 row tensor:
  // (uniform base) + (32-bit offset of the lane's 16 bytes of block 2w) + 64 q -- one register serves every tensor of a tile
  auto tile_row0 = [&](int gi, int r) -> int { return ((g0 + gi) * R + r) * 16; };
  // (derived from an OPAQUE copy of the lane id: the offsets of a group would otherwise be formed once and kept across its matrix
  // phases for the next boundary -- two registers per tile that the matrix phases do not have)
  auto row_off = [&](int r0) -> unsigned {
    const unsigned ln = ppr_opaque(lane);
    const int m = r0 + (int)(ln & 15);
    return (unsigned)((m < M) ? m : M - 1) * 512u + 64u * (2 * w) + 16u * (ln >> 4);
  };
  auto at = [](const float* base, unsigned off, int q) -> float* { return (float*)((char*)base + (size_t)off + 64 * q); };
  auto pk4 = [](const f32x4& b0, const f32x4& b1) -> u32x4 {
    return u32x4{pk_bf16(b0[0], b0[1]), pk_bf16(b0[2], b0[3]), pk_bf16(b1[0], b1[1]), pk_bf16(b1[2], b1[3])};
  };
  // ---- matrix phase: acc[r][q] = b_u + sum_j W_u[blocks, K-slice j] . x_j for the R tiles of a piece image (u = 0 / 1: the half's
  // first / second unit)
  auto matrix = [&](const u32x4 (&Wu)[3][2][4], int u, unsigned img) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < 2; ++q) acc[r][q] = *(lds_cf32x4*)ppr_lds(cq + u * 512 + 64 * q);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      lds_char* it = ppr_lds(img) + r * PPR_TILE_PIECES;
      u32x4 xb[2][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) xb[0][p] = *(lds_cu32x4*)(it + p * 1024);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j + 1 < 4) {
#pragma unroll
          for (int p = 0; p < 3; ++p) xb[(j + 1) & 1][p] = *(lds_cu32x4*)(it + ((j + 1) * 3 + p) * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
        const u32x4(&x)[3] = xb[j & 1];
        // gemm_q's term order: w3 x1, w2 x2, w2 x1, w1 x3, w1 x2, w1 x1
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[2][q][j], x[0], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[1][q][j], x[1], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[1][q][j], x[0], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[0][q][j], x[2], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[0][q][j], x[1], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[0][q][j], x[0], acc[r][q]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // ---- blocks 2w, 2w+1 of the R tiles (b[r][0..1], destroyed) -> K-slice w of a piece image: split_pair_mfma of mgn_x6.inc (the
  // remainders x - bf16(x) come from the matrix pipe), written out step by step and tile after tile: the two tiles' dependent
  // chains (convert, MFMA, convert, MFMA, convert) cover each other, every piece goes to LDS as soon as it exists, the
  // remainders replace the values in place.  The selector is re-made in every non-matrix phase: 8 registers that the matrix
  // phases need.
  // `hook(k)`, k = k0 .. k0 + 3R - 1: one memory instruction of the phase's DMA list per step -- issued back to back, eight LDS-DMA
  // instructions cost the wave ~190 cycles each (tools/timeline_ppr.py); between the conversions they queue behind nothing
  auto put_slices = [&](f32x4 (&b)[R][2], unsigned img, auto hook, int k0) {
    lds_char* o = ppr_lds(img) + (w * 3) * 1024;
    SplitSel S;  // (two LDS reads instead of ~22 vector instructions; not kept: 8 registers that the matrix phases need)
    {
      lds_char* sp = ppr_lds(sm0 + PPR_OFF_SEL + 16u * ppr_opaque(lane));
      S.s0 = *(lds_cu32x4*)sp;
      S.s1 = *(lds_cu32x4*)(sp + 1024);
    }
    PPR_STAMP(10);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const u32x4 x = pk4(b[r][0], b[r][1]);
        *(__attribute__((address_space(3))) u32x4*)(o + r * PPR_TILE_PIECES + p * 1024) = x;
        if (p < 2) {
          b[r][0] = MFMA_BF(S.s0, x, b[r][0]);
          b[r][1] = MFMA_BF(S.s1, x, b[r][1]);
        }
        hook(k0 + p * R + r);
        __builtin_amdgcn_sched_barrier(0);
      }
      PPR_STAMP(11 + p);
    }
  };
  // ---- boundary after a hidden layer l = 0..2 (its pre-activations are in acc): ReLU, saves, mask, operand of the next unit;
  // hook(0 .. 5R - 1)
  auto post_hidden = [&](int l, int gi, unsigned img_out, bool add_gathered, auto hook) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (add_gathered) {  // z0 = W_e e + b0 + Pd[dst] + Ps[src] (in k_mlp_fwd_x6's order of the two additions)
        constexpr int GO = 0;
        const f32x4 d0 = *(lds_cf32x4*)(ppr_lds(lq0) + GO + (r * 2 + 0) * 8192);
        const f32x4 d1 = *(lds_cf32x4*)(ppr_lds(lq1) + GO + (r * 2 + 0) * 8192);
        const f32x4 s0 = *(lds_cf32x4*)(ppr_lds(lq0) + GO + (r * 2 + 1) * 8192);
        const f32x4 s1 = *(lds_cf32x4*)(ppr_lds(lq1) + GO + (r * 2 + 1) * 8192);
        hook(2 * r);
        acc[r][0] += d0, acc[r][1] += d1;
        acc[r][0] += s0, acc[r][1] += s1;
      } else {
        hook(2 * r);
      }
      __builtin_amdgcn_sched_barrier(0);
      u32 bits = 0;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = acc[r][q][e];
          asm("v_max_f32 %0, 0, %0" : "+v"(v));
          acc[r][q][e] = v;
          if (TRAIN) {
            int t = __builtin_bit_cast(int, v);
            t = (t < 0) ? 0 : ((t > 1) ? 1 : t);
            bits |= (u32)t << (4 * q + e);
          }
        }
      hook(2 * r + 1);
      if (TRAIN) {
        const unsigned ro = row_off(tile_row0(gi, r));
        const float* sh = pick3(a.saveH[0], a.saveH[1], a.saveH[2], l);
#pragma unroll
        for (int q = 0; q < 2; ++q) ppr_st4_nt(at(sh, ro, q), acc[r][q]);
        // word g of row m holds bit 4 ib + e for feature 16 ib + 4 g + e: this wave's blocks are byte w of the word (byte 16 m + 4 g + w)
        const uint32_t* smk = pick3(a.saveM[0], a.saveM[1], a.saveM[2], l);
        *(__attribute__((address_space(1))) unsigned char*)((char*)smk + (size_t)(((ro >> 9) << 4) + 4 * g + w)) = (unsigned char)bits;
      }
      __builtin_amdgcn_sched_barrier(0);
      PPR_STAMP(8 + r);
    }
    put_slices(acc, img_out, hook, 2 * R);
  };

  // ===== both halves run ONE instruction stream (matrix, boundary, matrix, boundary per group; the differences sit behind wave-uniform
  // branches inside the non-matrix phases)
  const float* e_rows = a.src[0];
  const float *Pd = a.add_src[0], *Ps = a.add_src[1];
  const int32_t *dsti = a.add_idx[0], *srci = a.add_idx[1];
  // DMA shares of a wave (h = 0): instructions kk = 2w, 2w+1 of every 8 (rows 2kk, 2kk+1 of the tile); lane: row 2kk + (lane >> 5),
  // LDS slot s = lane & 31 of that row, which holds global chunk s ^ (row & 15)
  // The LDS-DMA instructions of a wave come in PAIRS (instructions kk = 2w, 2w + 1 of the eight of a tile: rows 4w .. 4w + 3, LDS
  // blocks kk and kk + 1).  Lane: row 2 kk + (lane >> 5), LDS slot s = lane & 31 of that row, which holds chunk s ^ (row & 15).
  // xo[k2] = byte offset of the lane's 16 bytes inside the tile for instruction k2 of the pair -- formed once per phase.
  struct DmaLane {
    unsigned xo[2];   // (4w + 2 k2 + rhalf) * 512 + 16 * chunk      (e rows: the tile is contiguous)
    unsigned xc[2];   // 16 * chunk                                   (gathered rows)
    int rhalf;
  };
  auto dma_lane = [&]() -> DmaLane {
    const unsigned ln = ppr_opaque(lane);
    DmaLane d;
    d.rhalf = ln >> 5;
    const unsigned sl = ln & 31;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const unsigned rit = 4 * w + 2 * k2 + d.rhalf;
      d.xc[k2] = 16u * (sl ^ (rit & 15));
      d.xo[k2] = rit * 512u + d.xc[k2];
    }
    return d;
  };
  // pair r of the R a wave contributes to a group's e rows (destination: the group's slot of the ring)
  auto dma_e2 = [&](const DmaLane& d, int gi, int r) {
    const unsigned dst_off = PPR_OFF_E + (unsigned)(gi % 3) * PPR_E_SLOT;   // (the slot of group gi - 3: its epilogue ran a phase ago)
    const int gc = (gi < ng) ? gi : ng - 1;  // past the end: the last group again (unconditional instructions, nobody reads it)
    const int r0 = tile_row0(gc, r);
    unsigned v0, v1;
    if (r0 + 16 <= M) {
      v0 = (unsigned)r0 * 512u + d.xo[0];
      v1 = (unsigned)r0 * 512u + d.xo[1];
    } else {  // the ragged last tile: rows clamped
      int m0 = r0 + 4 * w + d.rhalf, m1 = m0 + 2;
      m0 = (m0 < M) ? m0 : M - 1;
      m1 = (m1 < M) ? m1 : M - 1;
      v0 = (unsigned)m0 * 512u + d.xc[0];
      v1 = (unsigned)m1 * 512u + d.xc[1];
    }
    glds16x2(e_rows, v0, v1, sm0 + dst_off + r * 8192 + (2 * w) * 1024);
  };
  // the gathered rows of group gi: this wave's rows 4w .. 4w+3 of every tile; their indices are SCALAR loads (16 bytes of the
  // index arrays per tile and source: no vector register is held across a matrix phase for them)
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  auto load_gidx = [&](int gi, i32x4 (&iv)[R][2]) {
    const int gc = (gi < ng) ? gi : ng - 1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int mrow = tile_row0(gc, r) + 4 * w;
      if (mrow + 4 <= M) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
          iv[r][s] = *(const __attribute__((address_space(4))) i32x4*)(unsigned long long)((s ? srci : dsti) + mrow);
      } else {  // the ragged end: row by row, clamped
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int m = (mrow + e < M) ? mrow + e : M - 1;
            iv[r][s][e] = *(const __attribute__((address_space(4))) int*)(unsigned long long)((s ? srci : dsti) + m);
          }
      }
    }
  };
  // pair k = 2r + s of the 2R a wave contributes to a group's gathered rows (s = 0: Pd[dst], 1: Ps[src])
  auto dma_g2 = [&](const DmaLane& d, const i32x4 (&iv)[R][2], int k) {
    const int r = k >> 1, sx = k & 1;
    const int row0 = d.rhalf ? iv[r][sx][1] : iv[r][sx][0];
    const int row1 = d.rhalf ? iv[r][sx][3] : iv[r][sx][2];
    glds16x2(sx ? Ps : Pd, (unsigned)row0 * 512u + d.xc[0], (unsigned)row1 * 512u + d.xc[1], sm0 + PPR_OFF_G + (r * 2 + sx) * 8192 + (2 * w) * 1024);
  };
  auto split_e = [&](int gi, auto hook, int k0) {
    f32x4 b[R][2];
    const unsigned EO = eoff(gi);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      b[r][0] = *(lds_cf32x4*)(ppr_lds(lq0 + EO) + r * 8192);
      b[r][1] = *(lds_cf32x4*)(ppr_lds(lq1 + EO) + r * 8192);
    }
    put_slices(b, pA, hook, k0);  // (h = 0: pA = P)
  };
  int keyr[R], nbkr[R];  // h = 1: this lane's row key (-1 past M) and the keys either side of the tile, fetched two phases ahead
  auto load_keys = [&](int gi) {
    const int cc = ppr_opaque(lane) & 15;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int r0 = tile_row0(gi, r);
      if (r0 > 0 && r0 + 17 <= M) {  // an inner tile: nothing to clamp
        keyr[r] = dsti[r0 + cc];
        nbkr[r] = a.seg_key[(cc < 8) ? r0 - 1 : r0 + 16];
      } else {
        const int m = r0 + cc;
        const int k = dsti[(m < M) ? m : M - 1];
        keyr[r] = (m < M) ? k : -1;
        int rk = (cc < 8) ? r0 - 1 : r0 + 16;
        rk = (rk < 0) ? 0 : rk;
        rk = (rk < M) ? rk : M - 1;
        nbkr[r] = a.seg_key[rk];
      }
    }
  };
#pragma unroll
  for (int r = 0; r < R; ++r) keyr[r] = nbkr[r] = 0;
  // epilogue of group gi (z in acc, the rows' square sums in LDS): RMSNorm (reference epsilon placement), residual, stores, and the
  // fused aggregation of y over runs of equal keys (seg_scan_store<true> of mgn_x6.inc, this wave's two blocks)
  auto epilogue = [&](int gi) {
    // stage by stage over the R tiles (their dependent chains -- LDS read, square root, two divisions, products, four scan steps --
    // cover each other: tile after tile the phase took 1 400-1 800 cycles per tile)
    const unsigned EO = eoff(gi);
    float inv[R];
    unsigned ro[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ro[r] = row_off(tile_row0(gi, r));
      const f32x4 s4 = *(lds_cf32x4*)(sm + PPR_OFF_SSQ + (r * 16 + c) * 16);
      const float ss = ((s4[0] + s4[1]) + s4[2]) + s4[3];
      // (hardware square root and reciprocal, 1 ulp each: the IEEE sequences of the x6 kernels are ~45 vector instructions per
      // tile in a phase that is bound by its instruction count; 2e-7 against a 1e-5 parity bar)
      const float rms = __builtin_amdgcn_sqrtf(ss) * 0.08838834764831845f;  // / sqrt(128)
      inv[r] = __builtin_amdgcn_rcpf(rms + a.eps);
      if (TRAIN && w == 0 && g == 0) st1((float*)((char*)a.saveR + (size_t)((ro[r] >> 9) << 2)), rms);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 y[R][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const f32x4 sc4 = *(lds_cf32x4*)(ppr_lds(cq) + 2 * 512 + 64 * q);  // (h = 1: cq is at bias row 2; the scale is row 4)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const f32x4 u = acc[r][q] * inv[r];
        if (TRAIN) ppr_st4_nt(at(a.saveU, ro[r], q), u);
        y[r][q] = sc4 * u;
        const f32x4 er = *(lds_cf32x4*)(ppr_lds((q ? lq1 : lq0) + EO) + r * 8192);
        st4(at(a.out, ro[r], q), er + y[r][q]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    float same[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) pp_seg_same(same[r], keyr[r]);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) pp_seg_scan_blk(y[r][q], same[r]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int r0 = tile_row0(gi, r);
      const int key = keyr[r], nbk = nbkr[r];
      const int kprev = (r0 > 0) ? __builtin_amdgcn_readlane(nbk, 0) : -1;
      const int knxt = (r0 + 16 < M) ? __builtin_amdgcn_readlane(nbk, 15) : -1;
      const int knext = __builtin_amdgcn_update_dpp(-3, key, 0x101, 0xf, 0xf, false);  // row_shl:1, lane 15 keeps -3
      const int key0 = __builtin_amdgcn_readfirstlane(key);
      if (key >= 0 && knext != key) {  // run end
        const bool before = (key == key0) && (kprev == key0);
        const bool inside = !before && !(knext == -3 && knxt == key);
        float* dst = inside ? a.seg_out + (long)key * H : a.seg_part + ((long)(r0 >> 4) * 2 + (before ? 0 : 1)) * H;
#pragma unroll
        for (int q = 0; q < 2; ++q) st4(dst + 16 * (2 * w + q) + 4 * g, y[r][q]);
      }
      __builtin_amdgcn_sched_barrier(0);
      PPR_STAMP(14 + r);
    }
  };

  // ---- prologue: group 0's rows (h = 0); the second half starts five phases later
  auto nohook = [](int) {};
  if (h == 0) {
    i32x4 iv[R][2];
    load_gidx(0, iv);
    const DmaLane d = dma_lane();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      dma_e2(d, 0, r);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < 2 * R; ++k) {
      dma_g2(d, iv, k);
      __builtin_amdgcn_sched_barrier(0);
    }
    dma_drain();
  }
  ppr_barrier();
  if (h == 0) {
    split_e(0, nohook, 0);
  } else {
#pragma unroll 1
    for (int k = 0; k < 5; ++k) {
      ppr_barrier();
      if (GH1 && k == 2) {  // phase 2: group 0's gathered rows have been read (phase 1); group 1's are needed in phase 5
        i32x4 iv1[R][2];
        load_gidx(1, iv1);
        const DmaLane d = dma_lane();
#pragma unroll
        for (int kk = 0; kk < 2 * R; ++kk) {
          dma_g2(d, iv1, kk);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (GH1 && k == 3) dma_drain();
    }
  }
#pragma unroll 1
  for (int gi = 0; gi < ng; ++gi) {
    // ================= first unit of the half (h = 0: W_e . e; h = 1: layer 2)
    PPR_STAMP(0);
    ppr_barrier();
    PPR_STAMP(1);
    matrix(W[0], 0, pA);
    // the gathered rows of this group have landed: their LDS-DMAs were issued before the six stores (TRAIN) of that boundary
    if (!GH1 && h == 0) {
      if (TRAIN) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    PPR_STAMP(2);
    ppr_barrier();
    PPR_STAMP(3);
    // boundary of layer 2h; spread through it: h = 0 the next group's e rows (R LDS-DMA pairs), GH1: h = 1 the gathered rows of group
    // gi + 2 (2R pairs) -- TRAIN: all issued before the boundary's first store
    if (h) load_keys(gi);
    i32x4 ivg[R][2];  // GH1, h = 1: the gather indices of group gi + 2 (scalar loads: landed by the time the second hook needs them; held
    if (GH1 && h) load_gidx(gi + 2, ivg);   // across the matrix phase before, they cost 16 scalar registers the kernel does not have)
    {
      const DmaLane d = dma_lane();
      // TRAIN: hooks 0 and 1, before the boundary's first store (the counted waits then leave all six stores in flight); inference:
      // hooks 0 and 2, apart from each other (back to back they cost ~3 us per launch)
      post_hidden(2 * h, gi, pB, h == 0, [&](int k) {
        if (h) {  // GH1: the four gather pairs of group gi + 2, TRAIN all before the first store (hook 0), inference one per hook
          if (GH1) {
            if (TRAIN) {
              if (k == 0) {
#pragma unroll
                for (int kk = 0; kk < 2 * R; ++kk) dma_g2(d, ivg, kk);
              }
            } else if (k < 2 * R) {
              dma_g2(d, ivg, k);
            }
          }
          return;
        }
        const int r = TRAIN ? k : (k >> 1);
        if (r < R && (TRAIN || (k & 1) == 0)) dma_e2(d, gi + 1, r);
      });  // TRAIN: 6 stores
    }
    // ================= second unit of the half (h = 0: layer 1; h = 1: layer 3)
    PPR_STAMP(4);
    ppr_barrier();
    PPR_STAMP(5);
    i32x4 iv[R][2];  // !GH1, h = 0: the next group's gather indices -- scalar loads issued here, used by the boundary after this matrix phase
    if (!GH1 && h == 0) load_gidx(gi + 1, iv);
    matrix(W[1], 1, pB);
    // h = 0: the next group's e rows, asked for in the boundary phase, have landed: their LDS-DMAs were issued before the boundary's six
    // stores (TRAIN), which may stay in flight.  (GH1: the second half's gather pairs have until the end of its epilogue phase.)
    if (h == 0) {
      if (TRAIN) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (h) {
      // z is complete: this wave's share of every row's sum of squares
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float ss = 0.f;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) ss = fmaf(acc[r][q][e], acc[r][q][e], ss);
        ss = pp_rowsum4(ss);
        if (g == 0) *(__attribute__((address_space(3))) float*)(sm + PPR_OFF_SSQ + (r * 16 + c) * 16 + 4 * w) = ss;
      }
    }
    PPR_STAMP(6);
    ppr_barrier();
    PPR_STAMP(7);
    if (h == 0) {
      // boundary of layer 1 -> Qin, then the next group's e rows -> P; the next group's gathered rows (4R LDS-DMA instructions)
      // spread through both
      if constexpr (GH1) {
        post_hidden(1, gi, pA + (PPR_OFF_QIN - PPR_OFF_P), false, nohook);  // TRAIN: 6 stores
        split_e(gi + 1, nohook, 0);
      } else {
      const DmaLane d = dma_lane();
      auto hk = [&](int k) {  // TRAIN: hooks 0 and 1 (two pairs each), before the boundary's first store; inference: hooks 0 .. 3
        if (TRAIN) {
          if (k < R) {
            dma_g2(d, iv, 2 * k);
            dma_g2(d, iv, 2 * k + 1);
          }
        } else if (k < 2 * R) {
          dma_g2(d, iv, k);
        }
      };
      post_hidden(1, gi, pA + (PPR_OFF_QIN - PPR_OFF_P), false, hk);  // hooks 0 .. 5R-1; TRAIN: 6 stores
      split_e(gi + 1, hk, 5 * R);
      }
    } else {
      epilogue(gi);
      // GH1: the gathered rows of group gi + 2 (asked for two phases ago) have landed: younger are the 6 stores of that boundary (TRAIN)
      // and at least the 2R (inference) / 4R (TRAIN) row stores of this epilogue
      if (GH1) {
        if (TRAIN) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      }
    }
  }
  if (h == 0) {  // five more phases: the other half drains its pipeline
#pragma unroll 1
    for (int k = 0; k < 5; ++k) ppr_barrier();
  }
  PPR_TL_DUMP();
}

// ============================================================================================================================
// The edge BACKWARD chain in the same shape (k_mlp_bwd_x6<6, false, 0, false, SbEdge>: RMSNorm backward, three masked input-
// gradient products, dE = resid + W_e^T dz0; column sums: dscale only).  Units in the stream order of mgn_mlp_bwd_args.wpk:
// WT[3], WT[2] (waves h = 0), WT[1], WT0[0] (waves h = 1); every wave owns 32 of the 128 features of each row.
//
//   phase        4g           4g+1                   4g+2         4g+3
//   h = 0     GEMM WT3     dz2 = mask2, dZ[2]      GEMM WT2     dz1 = mask1, dZ[1] -> Qin;  dz3 of group g+1 -> dZ[3], P
//   phase        4g+5         4g+6                   4g+7         4g+8
//   h = 1     GEMM WT1     resid(g) asked for;      GEMM WT0     rows of group g+3 asked for;
//                          dz0 = mask0, dZ[0];                   dE(g) = resid + acc
//                          row dots + dscale of group g+2
//
// RMSNorm backward needs a full-row product <scale dY, U> before any wave can form its 32 features of dz3: the h = 1 waves
// compute the four partial products of a row (and the dscale column sums) one boundary earlier and leave them in LDS, the h = 0
// waves read them when they form dz3.  All LDS-DMA is issued by the h = 1 waves: the rows of a group (dOut, dOut2[idx2], U:
// 48 KB for two tiles), its three mask words and rms (global_load_lds_dword, 256 bytes per tile and array), and dOut once more
// for the residual of dE.  Rows past M are computed as copies of row M - 1 and stored there again; they are left out of dscale.
// dZ[2..0] and dE run gemm_q's term order on the mgn_wpack image; dz3 adds its row product in another order than the x6 kernel
// (4 partial sums of 32) and uses the hardware reciprocal: results agree to rounding (~1e-7), not bit for bit.

#define PPB_OFF_LAND (3 * PPR_IMG)                      /* dOut | dOut2[idx2] | U rows of a group */
#define PPB_OFF_RES (PPB_OFF_LAND + 3 * PPR_R * 8192)   /* the residual rows (dOut once more) */
#define PPB_OFF_CST (PPB_OFF_RES + PPR_R * 8192)        /* scale */
#define PPB_OFF_MASK (PPB_OFF_CST + 512)                /* ring of 4 groups x R tiles x 3 layers x 256 bytes */
#define PPB_OFF_RMS (PPB_OFF_MASK + 4 * PPR_R * 3 * 256)
#define PPB_OFF_DOT (PPB_OFF_RMS + PPR_R * 256)         /* [tile][row][wave] partial row products */
#define PPB_OFF_DSC (PPB_OFF_DOT + PPR_R * 256)         /* dscale accumulators [128] */
#define PPB_OFF_SEL (PPB_OFF_DSC + 512)
#define PPB_LDS_BYTES (PPB_OFF_SEL + 2048)

// one LDS-DMA of 256 bytes: lane L fetches 4 bytes at sbase + voff(L) into LDS byte lds_addr + 4 L
__device__ __forceinline__ void glds4(const void* sbase, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_addr)
      : "memory");
}

template <bool XCD>
__global__ void __launch_bounds__(512, 2) k_edge_bwd_ppr(const mgn_mlp_bwd_args a, const int nred) {
  constexpr int H = 128, R = PPR_R, NSLOT = 5;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* sm = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = wave >> 2, w = wave & 3;
  const int c = lane & 15, g = lane >> 4;
  const unsigned sm0 = __builtin_amdgcn_readfirstlane(lds_addr_of(sm));
  PPR_TL_DECL();
  const int M = (int)a.M;
  const int T = (M + 15) / 16;
  const int NG = (T + R - 1) / R;
  const int G = gridDim.x;
  const int per = (NG + G - 1) / G;
  int cb = blockIdx.x;
  if (XCD && (G & 7) == 0) cb = (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3);
  const int g0 = cb * per;
  const int g1 = (g0 + per < NG) ? g0 + per : NG;
  const int ng = (g1 > g0) ? g1 - g0 : 0;
  float* ws = (float*)a.red_ws;
  // the column-sum partials of workgroups that do not exist (the reduction reads nred of them)
  for (int b = blockIdx.x + G; b < nred; b += G)
    for (int i = threadIdx.x; i < H; i += 512) ws[((size_t)b * NSLOT + 4) * H + i] = 0.f;
  if (ng == 0) {
    for (int i = threadIdx.x; i < H; i += 512) ws[((size_t)blockIdx.x * NSLOT + 4) * H + i] = 0.f;
    return;
  }

  u32x4 W[2][3][2][4];
  {
    const char* wb = (const char*)a.wpk[0] + (size_t)(2 * h) * MGN_WPACK_BYTES + (size_t)(2 * w) * 1024 + 16u * lane;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            W[u][p][q][j] = *(const __attribute__((address_space(1))) u32x4*)(wb + (size_t)u * MGN_WPACK_BYTES + j * X6_QBYTES + p * 8192 + q * 1024);
  }
  for (int i = threadIdx.x; i < H; i += 512) {
    ((__attribute__((address_space(3))) float*)(sm + PPB_OFF_CST))[i] = a.scale[i];
    ((__attribute__((address_space(3))) float*)(sm + PPB_OFF_DSC))[i] = 0.f;
  }
  if (wave == 0) {
    const SplitSel S0 = split_sel<true>();
    *(__attribute__((address_space(3))) u32x4*)(sm + PPB_OFF_SEL + 16 * lane) = S0.s0;
    *(__attribute__((address_space(3))) u32x4*)(sm + PPB_OFF_SEL + 1024 + 16 * lane) = S0.s1;
  }
  // per-lane LDS addresses (see the forward kernel): piece images, the lane's 16 bytes of blocks 2w / 2w+1 of a landed tile
  const unsigned pA = ppr_opaque(sm0 + (h ? PPR_OFF_QIN : PPR_OFF_P) + 16u * lane);
  const unsigned pB = ppr_opaque(sm0 + (h ? PPR_OFF_QOWN : PPR_OFF_P) + 16u * lane);
  const unsigned lq0 = ppr_opaque(sm0 + PPB_OFF_LAND + c * 512 + 16 * ((4 * (2 * w) + g) ^ c));
  const unsigned lq1 = ppr_opaque(sm0 + PPB_OFF_LAND + c * 512 + 16 * ((4 * (2 * w + 1) + g) ^ c));
  f32x4 acc[R][2];

  auto tile_row0 = [&](int gi, int r) -> int { return ((g0 + gi) * R + r) * 16; };
  auto row_off = [&](int r0) -> unsigned {
    const unsigned ln = ppr_opaque(lane);
    const int m = r0 + (int)(ln & 15);
    return (unsigned)((m < M) ? m : M - 1) * 512u + 64u * (2 * w) + 16u * (ln >> 4);
  };
  auto at = [](const float* base, unsigned off, int q) -> float* { return (float*)((char*)base + (size_t)off + 64 * q); };
  auto pk4 = [](const f32x4& b0, const f32x4& b1) -> u32x4 {
    return u32x4{pk_bf16(b0[0], b0[1]), pk_bf16(b0[2], b0[3]), pk_bf16(b1[0], b1[1]), pk_bf16(b1[2], b1[3])};
  };
  auto matrix = [&](const u32x4 (&Wu)[3][2][4], unsigned img) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < 2; ++q) acc[r][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < R; ++r) {
      lds_char* it = ppr_lds(img) + r * PPR_TILE_PIECES;
      u32x4 xb[2][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) xb[0][p] = *(lds_cu32x4*)(it + p * 1024);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j + 1 < 4) {
#pragma unroll
          for (int p = 0; p < 3; ++p) xb[(j + 1) & 1][p] = *(lds_cu32x4*)(it + ((j + 1) * 3 + p) * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
        const u32x4(&x)[3] = xb[j & 1];
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[2][q][j], x[0], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[1][q][j], x[1], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[1][q][j], x[0], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[0][q][j], x[2], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[0][q][j], x[1], acc[r][q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = MFMA_BF(Wu[0][q][j], x[0], acc[r][q]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  auto put_slices = [&](f32x4 (&b)[R][2], unsigned img) {
    lds_char* o = ppr_lds(img) + (w * 3) * 1024;
    SplitSel S;
    {
      lds_char* sp = ppr_lds(sm0 + PPB_OFF_SEL + 16u * ppr_opaque(lane));
      S.s0 = *(lds_cu32x4*)sp;
      S.s1 = *(lds_cu32x4*)(sp + 1024);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const u32x4 x = pk4(b[r][0], b[r][1]);
        *(__attribute__((address_space(3))) u32x4*)(o + r * PPR_TILE_PIECES + p * 1024) = x;
        if (p < 2) {
          b[r][0] = MFMA_BF(S.s0, x, b[r][0]);
          b[r][1] = MFMA_BF(S.s1, x, b[r][1]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // boundary of a chain unit: dz_{l-1} = acc masked by the ReLU bits of layer l's input (mask layer ml = l - 1), stored to dZ[ml],
  // split into the operand of the next unit
  auto post_masked = [&](int ml, int gi, unsigned img_out) {
    float* dzp = pick3(a.dZ[0], a.dZ[1], a.dZ[2], ml);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned lnq = ppr_opaque(lane);
      const unsigned bits = *(__attribute__((address_space(3))) const unsigned char*)(sm + PPB_OFF_MASK + (((g0 + gi) & 3) * R + r) * 768 + ml * 256 +
                                                                                         (lnq & 15) * 16 + 4 * (lnq >> 4) + w);
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = ((int)(bits << (31 - (4 * q + e)))) >> 31;  // v_bfe_i32: all ones where the bit is set
          const float v = acc[r][q][e];  // (a scalar copy first: __builtin_bit_cast of a vector ELEMENT reads element 0)
          acc[r][q][e] = __builtin_bit_cast(float, __builtin_bit_cast(int, v) & t);
        }
      const unsigned ro = row_off(tile_row0(gi, r));
#pragma unroll
      for (int q = 0; q < 2; ++q) ppr_st4_nt(at(dzp, ro, q), acc[r][q]);
      __builtin_amdgcn_sched_barrier(0);
    }
    put_slices(acc, img_out);
  };
  // ---- LDS-DMA lists of the h = 1 waves (pairs: see the forward kernel)
  struct DmaLane {
    unsigned xo[2], xc[2];
    int rhalf;
  };
  auto dma_lane = [&]() -> DmaLane {
    const unsigned ln = ppr_opaque(lane);
    DmaLane d;
    d.rhalf = ln >> 5;
    const unsigned sl = ln & 31;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const unsigned rit = 4 * w + 2 * k2 + d.rhalf;
      d.xc[k2] = 16u * (sl ^ (rit & 15));
      d.xo[k2] = rit * 512u + d.xc[k2];
    }
    return d;
  };
  auto clampg = [&](int gi) -> int { return (gi < 0) ? 0 : ((gi < ng) ? gi : ng - 1); };
  // this wave's pair of a contiguous 16-row tile of `base` (row r0 + ...) -> LDS block pair 2w of the tile at dst_off
  auto dma_tile = [&](const DmaLane& d, const float* base, int r0, unsigned dst_off) {
    unsigned v0, v1;
    if (r0 + 16 <= M) {
      v0 = (unsigned)r0 * 512u + d.xo[0];
      v1 = (unsigned)r0 * 512u + d.xo[1];
    } else {
      int m0 = r0 + 4 * w + d.rhalf, m1 = m0 + 2;
      m0 = (m0 < M) ? m0 : M - 1;
      m1 = (m1 < M) ? m1 : M - 1;
      v0 = (unsigned)m0 * 512u + d.xc[0];
      v1 = (unsigned)m1 * 512u + d.xc[1];
    }
    glds16x2(base, v0, v1, sm0 + dst_off + (2 * w) * 1024);
    __builtin_amdgcn_sched_barrier(0);
  };
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  // everything of group gi that the RMSNorm backward and the masks need: dOut, dOut2[idx2], U rows; mask words (wave w < 3: layer w);
  // rms (wave 3)
  auto dma_rows = [&](int gi) {
    const int gc = clampg(gi);
    const DmaLane d = dma_lane();
    i32x4 iv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int mrow = tile_row0(gc, r) + 4 * w;
      if (mrow + 4 <= M) {
        iv[r] = *(const __attribute__((address_space(4))) i32x4*)(unsigned long long)(a.idx2 + mrow);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = (mrow + e < M) ? mrow + e : M - 1;
          iv[r][e] = *(const __attribute__((address_space(4))) int*)(unsigned long long)(a.idx2 + m);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int r0 = tile_row0(gc, r);
      dma_tile(d, a.dOut, r0, PPB_OFF_LAND + r * 8192);
      dma_tile(d, a.U, r0, PPB_OFF_LAND + (2 * R + r) * 8192);
      const int row0 = d.rhalf ? iv[r][1] : iv[r][0];
      const int row1 = d.rhalf ? iv[r][3] : iv[r][2];
      glds16x2(a.dOut2, (unsigned)row0 * 512u + d.xc[0], (unsigned)row1 * 512u + d.xc[1], sm0 + PPB_OFF_LAND + (R + r) * 8192 + (2 * w) * 1024);
      __builtin_amdgcn_sched_barrier(0);
      const unsigned ln = ppr_opaque(lane);
      if (w < 3) {  // 16 rows x 16 bytes of mask words, contiguous
        int m = r0 + (int)(ln >> 2);
        m = (m < M) ? m : M - 1;
        glds4(pick3(a.Ms[0], a.Ms[1], a.Ms[2], w), (unsigned)m * 16u + 4u * (ln & 3), sm0 + PPB_OFF_MASK + (((g0 + gc) & 3) * R + r) * 768 + w * 256);
      } else {
        int m = r0 + (int)(ln & 15);
        m = (m < M) ? m : M - 1;
        glds4(a.R, (unsigned)m * 4u, sm0 + PPB_OFF_RMS + r * 256);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto dma_resid = [&](int gi) {
    const int gc = clampg(gi);
    const DmaLane d = dma_lane();
#pragma unroll
    for (int r = 0; r < R; ++r) dma_tile(d, a.din_resid[0], tile_row0(gc, r), PPB_OFF_RES + r * 8192);
  };
  // ---- h = 1: the partial row products <scale dY, U> of group gi (this wave's 32 features) -> LDS, and its share of dscale
  auto row_dots = [&](int gi) {
    // block by block (4 accumulators of dscale live at a time, not 8: with both blocks in flight the phase spilled five weight
    // fragments, whose reloads in the matrix phase wait for every store in flight)
    const float ones[4] = {1.f, 1.f, 1.f, 1.f};
    float dp[R];
    float keep[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      dp[r] = 0.f;
      keep[r] = (tile_row0(gi, r) + (int)(ppr_opaque(lane) & 15) < M) ? 1.f : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x4 vs = {0.f, 0.f, 0.f, 0.f};
      const f32x4 sc = *(lds_cf32x4*)(sm + PPB_OFF_CST + 64 * (2 * w + q) + 16 * g);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        lds_char* lp = ppr_lds(q ? lq1 : lq0) + r * 8192;
        const f32x4 dy = *(lds_cf32x4*)lp + *(lds_cf32x4*)(lp + R * 8192);
        const f32x4 u = *(lds_cf32x4*)(lp + 2 * R * 8192);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vs[e] = fmaf(dy[e] * keep[r], u[e], vs[e]);
          dp[r] = fmaf(sc[e] * dy[e], u[e], dp[r]);
        }
        // (pinned HERE: machine sinking otherwise moves the row product down to its use after the scan, and the rows it reads stay
        // live across it -- five weight fragments spilled)
        asm volatile("" : "+v"(dp[r]), "+v"(vs));
        __builtin_amdgcn_sched_barrier(0);
      }
      // sum over the 16 rows (an inclusive DPP scan leaves the total in lane 15 of every row of lanes), then onto the wave's own
      // accumulators in LDS (no other wave touches them)
      pp_seg_scan_blk(vs, ones);
      if (c == 15) {
        __attribute__((address_space(3))) f32x4* dp4 = (__attribute__((address_space(3))) f32x4*)(sm + PPB_OFF_DSC + 64 * (2 * w + q) + 16 * g);
        *dp4 = *dp4 + vs;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float t = pp_rowsum4(dp[r]);
      if (g == 0) *(__attribute__((address_space(3))) float*)(sm + PPB_OFF_DOT + (r * 16 + c) * 16 + 4 * w) = t;
    }
  };
  // ---- h = 0: dz3 of group gi (this wave's 32 features) from the landed rows and the row products: stored to dZ[3], split -> P
  //      dz = g / (rms + eps) - u <g, u> / (H rms),  g = scale dY
  auto form_dz3 = [&](int gi) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int cc = ppr_opaque(lane) & 15;
      const f32x4 s4 = *(lds_cf32x4*)(sm + PPB_OFF_DOT + (r * 16 + cc) * 16);
      const float dot = ((s4[0] + s4[1]) + s4[2]) + s4[3];
      const float rms = *(__attribute__((address_space(3))) const float*)(sm + PPB_OFF_RMS + r * 256 + 4 * cc);
      const float inv = __builtin_amdgcn_rcpf(rms + a.eps);
      const float k2 = (rms > 0.f) ? dot * __builtin_amdgcn_rcpf((float)H * rms) : 0.f;
      const unsigned ro = row_off(tile_row0(gi, r));
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        lds_char* lp = ppr_lds(q ? lq1 : lq0) + r * 8192;
        const f32x4 dy = *(lds_cf32x4*)lp + *(lds_cf32x4*)(lp + R * 8192);
        const f32x4 u = *(lds_cf32x4*)(lp + 2 * R * 8192);
        const f32x4 sc = *(lds_cf32x4*)(sm + PPB_OFF_CST + 64 * (2 * w + q) + 16 * g);
        acc[r][q] = (sc * dy) * inv - u * k2;
        ppr_st4_nt(at(a.dZ[3], ro, q), acc[r][q]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    put_slices(acc, sm0 + PPR_OFF_P + 16u * ppr_opaque(lane));
  };

  // ---- start-up: rows of group 0, its row products, dz3(0); rows of group 1
  if (h) {
    dma_rows(0);
    dma_drain();
  }
  ppr_barrier();
  if (h) row_dots(0);
  ppr_barrier();
  if (h == 0) form_dz3(0);
  ppr_barrier();
  if (h) {
    dma_rows(1);
    dma_drain();
  }
  ppr_barrier();
  if (h) ppr_barrier();  // phase 0: the second half starts five phases behind, with an iteration "-1" that only prepares
#pragma unroll 1
  for (int it = 0; it < ng + h; ++it) {
    const int gi = it - h;          // h = 1: iterations -1 .. ng - 1
    const bool act = gi >= 0;
    // ================= first unit of the half (h = 0: WT3; h = 1: WT1)
    PPR_STAMP(0);
    ppr_barrier();
    PPR_STAMP(1);
    if (act) matrix(W[0], pA);
    if (h) {  // the rows asked for in the previous boundary (group gi + 2) have landed; only the 2R stores of dE are younger
      if (gi >= 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    PPR_STAMP(2);
    ppr_barrier();
    PPR_STAMP(3);
    if (h == 0) {
      post_masked(2, gi, pB);
    } else {
      dma_resid(gi);
      PPR_STAMP(8);
      if (act) post_masked(0, gi, pB);
      PPR_STAMP(9);
      if (gi + 2 < ng) row_dots(gi + 2);
    }
    // ================= second unit of the half (h = 0: WT2; h = 1: WT0 = W_e^T)
    PPR_STAMP(4);
    ppr_barrier();
    PPR_STAMP(5);
    if (act) matrix(W[1], pB);
    if (h) {  // the residual rows have landed; only the 2R stores of dZ[0] are younger
      if (act) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    PPR_STAMP(6);
    ppr_barrier();
    PPR_STAMP(7);
    if (h == 0) {
      post_masked(1, gi, pA + (PPR_OFF_QIN - PPR_OFF_P));
      PPR_STAMP(8);
      if (gi + 1 < ng) form_dz3(gi + 1);
    } else {
      dma_rows(gi + 3);
      PPR_STAMP(8);
      if (act) {  // dE = resid + W_e^T dz0
        constexpr int RO = PPB_OFF_RES - PPB_OFF_LAND;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const unsigned ro = row_off(tile_row0(gi, r));
#pragma unroll
          for (int q = 0; q < 2; ++q) ppr_st4_nt(at(a.dIn[0], ro, q), *(lds_cf32x4*)(ppr_lds(q ? lq1 : lq0) + RO + r * 8192) + acc[r][q]);
        }
      }
    }
  }
  if (h == 0) {
#pragma unroll 1
    for (int k = 0; k < 5; ++k) ppr_barrier();
  }
  PPR_TL_DUMP();
  // the workgroup's dscale partial
  ppr_barrier();
  for (int i = threadIdx.x; i < H; i += 512)
    ws[((size_t)blockIdx.x * NSLOT + 4) * H + i] = ((__attribute__((address_space(3))) const float*)(sm + PPB_OFF_DSC))[i];
}
