// MI355X (gfx950) random extra edges: what the reference's Dataset does per sample when the config sets
// dataset.new_edges_ratio (graphphysics/dataset/dataset.py:171-203, torch_geometric.utils.add_random_edge(edge_index, p,
// force_undirected=True) of torch-geometric 2.6): K = round(E p) // 2 random node pairs that are not yet edges, appended in both
// directions.  Integer work only; the stream is counter-based (include/mgn_hip.h, mgn_randedge), so the result is pinned bit for
// bit.  Eighth translation unit of libmgn_hip.so.  This file is the SPARSE regime, 4 (E + K) <= N (N - 1) / 2; toy graphs
// denser than that are sampled by enumeration in preprocess.add_random_edges.
//
//   table   ONE open-addressing table (linear probing, 64-bit atomicCAS on the pair code lo * N + hi, 32-bit value) holds the
//           occupied pairs AND the candidates: value 0 = a pair of the input, value g + 1 = the lowest global candidate number
//           g = round * M + index that drew the pair (atomicMin).  A candidate is kept iff the value under its code is its own
//           g + 1: that one comparison says "not occupied, not drawn in an earlier round, first of its round".  Which SLOT a
//           code lands in depends on scheduling, the value under a code does not: min and "0 wins" commute.  Chosen over a
//           sorted occupied table plus a (code, index) sort per round: no sort of E codes per sample, no sort that would run
//           in rounds that have nothing to do (all rounds are queued), one lookup instead of two binary searches per candidate.
//   input   one pass over the input: copy both rows to the head of the output, range-check, insert the non-loop pairs.
//   round   x RE_ROUNDS, all queued, each kernel leaves at once when the running count cnt[r] has reached K:
//     cand  one thread per candidate: Philox, multiply-shift map to (a, b), reject a == b, insert, atomicMin.
//     flag  one workgroup per RE_BLOCK consecutive candidates: kept bit (value == g + 1) written back into the candidate
//           record, kept candidates of the workgroup counted with __ballot / popcount.
//     scan  ONE workgroup: exclusive scan of the (M / 2048, so a few hundred) workgroup counts, on top of cnt[r];
//           cnt[r + 1] = min(K, cnt[r] + total); after the last round a shortfall sets the error flag.  Done here, not by
//           rocPRIM: the base offset, the truncation at K and the shortfall flag ride along, and a round that has nothing to do
//           costs one load.
//     fill  the same workgroups: slot = offs[block] + rank (the ordered stream compaction of mgn_graphprim.inc); slots < K are
//           written to both new column blocks.  Acceptance order is (round, candidate index) order, never sorted-code order,
//           and bit-identical from run to run.
#include "mgn_hip.h"
#include "mgn_host.inc"       // g_err, fail, check_launch, workspace carving
#include "mgn_graphprim.inc"  // wave_kept, block_kept, block_compact_slot
#include "mgn_philox.inc"

extern "C" const char* mgn_randedge_last_error(void) { return g_err; }

#define RE_THREADS 256
#define RE_ITEMS 8
#define RE_BLOCK (RE_THREADS * RE_ITEMS)  // candidates one workgroup compacts
#define RE_ROUNDS MGN_RANDEDGE_ROUNDS
#define RE_NMAX 2147483647LL         // N, E < 2^31
#define RE_MMAX ((1LL << 30) - 1)    // RE_ROUNDS * M + 1 fits the 32-bit value of the table
#define RE_CAPMAX (1LL << 31)        // slots are stored as uint32
#define RE_EMPTY 0xffffffffffffffffull
#define RE_KEY_TWEAK 0x45444745u     // "EDGE": keeps this stream apart from mgn_add_noise's of the same seed and step

// ---------------------------------------------------------------------------------------- the table
__device__ __forceinline__ uint64_t re_mix(uint64_t x) {  // the 64-bit finaliser of MurmurHash3
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// slot of `code`, inserted if absent; -1 if the probe ran through the whole table (the host sizes it so that it cannot)
__device__ __forceinline__ int64_t re_slot(unsigned long long* __restrict__ keys, uint64_t mask, uint64_t code) {
  uint64_t s = re_mix(code) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[s], (unsigned long long)RE_EMPTY, (unsigned long long)code);
    if (prev == RE_EMPTY || prev == code) return (int64_t)s;
    s = (s + 1) & mask;
  }
  return -1;
}

// ---------------------------------------------------------------------------------------- input pass
__global__ void __launch_bounds__(256) k_re_input(const int64_t* __restrict__ row0, const int64_t* __restrict__ row1, long E, long N,
                                                  int64_t* __restrict__ out0, int64_t* __restrict__ out1,
                                                  unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, uint64_t mask,
                                                  int* __restrict__ flags) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t a = row0[e], b = row1[e];
  out0[e] = a;  // the input columns come first, untouched
  out1[e] = b;
  if (a < 0 || a >= N || b < 0 || b >= N) {  // not followed; reported through the deferred flag
    atomicOr(flags, MGN_RANDEDGE_ERR_RANGE);
    return;
  }
  if (a == b) return;  // a self loop occupies nothing
  const uint64_t code = (uint64_t)(a < b ? a : b) * (uint64_t)N + (uint64_t)(a < b ? b : a);
  const int64_t s = re_slot(keys, mask, code);
  if (s < 0) {
    atomicOr(flags, MGN_RANDEDGE_ERR_TABLE);
    return;
  }
  vals[s] = 0u;  // occupied: below every candidate's g + 1 (duplicates and (j, i) store the same 0)
}

// ---------------------------------------------------------------------------------------- one round
__global__ void __launch_bounds__(256) k_re_cand(int r, long M, long N, long K, uint32_t k0, uint32_t k1, uint32_t offset,
                                                 const int64_t* __restrict__ cnt, unsigned long long* __restrict__ keys,
                                                 uint32_t* __restrict__ vals, uint64_t mask, int32_t* __restrict__ lo,
                                                 int32_t* __restrict__ hi, uint32_t* __restrict__ slot, int* __restrict__ flags) {
  if (cnt[r] >= K) return;  // an earlier round filled the quota
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= M) return;
  uint32_t r0, r1;
  philox4x32_10(k0, k1, (uint32_t)c, (uint32_t)((uint64_t)c >> 32), (uint32_t)r, offset, r0, r1);
  const uint32_t a = (uint32_t)(((uint64_t)r0 * (uint64_t)N) >> 32), b = (uint32_t)(((uint64_t)r1 * (uint64_t)N) >> 32);
  int32_t l = -1, h = 0;
  uint32_t s = 0;
  if (a != b) {
    l = (int32_t)(a < b ? a : b), h = (int32_t)(a < b ? b : a);
    const int64_t at = re_slot(keys, mask, (uint64_t)l * (uint64_t)N + (uint64_t)h);
    if (at < 0) {
      atomicOr(flags, MGN_RANDEDGE_ERR_TABLE);
      l = -1;
    } else {
      s = (uint32_t)at;
      atomicMin(&vals[s], (uint32_t)((long)r * M + c + 1));
    }
  }
  lo[c] = l, hi[c] = h, slot[c] = s;
}

// thread t of pass p looks at candidate block * RE_BLOCK + p * RE_THREADS + t: a wave reads 64 consecutive candidates
__global__ void __launch_bounds__(RE_THREADS) k_re_flag(int r, long M, long K, const int64_t* __restrict__ cnt,
                                                        int32_t* __restrict__ lo, const uint32_t* __restrict__ slot,
                                                        const uint32_t* __restrict__ vals, uint32_t* __restrict__ blkcnt) {
  if (cnt[r] >= K) return;
  const long base = (long)blockIdx.x * RE_BLOCK;
  unsigned kept = 0;  // wave-uniform
  for (int p = 0; p < RE_ITEMS; ++p) {
    const long c = base + (long)p * RE_THREADS + threadIdx.x;
    bool keep = false;
    if (c < M && lo[c] >= 0) {
      keep = vals[slot[c]] == (uint32_t)((long)r * M + c + 1);
      if (!keep) lo[c] = -1;
    }
    kept += wave_kept(keep);
  }
  const unsigned t = block_kept<RE_THREADS>(kept);
  if (threadIdx.x == 0) blkcnt[blockIdx.x] = t;
}

// one workgroup: offs[b] = cnt[r] + sum of blkcnt[0 .. b)
__global__ void __launch_bounds__(256) k_re_scan(int r, long nb, long K, int64_t* __restrict__ cnt, const uint32_t* __restrict__ blkcnt,
                                                 int64_t* __restrict__ offs, int* __restrict__ flags) {
  __shared__ int64_t s_sum[256];
  const int64_t base = cnt[r];
  if (base >= K) {
    if (threadIdx.x == 0) cnt[r + 1] = base;
    return;
  }
  const long per = (nb + 255) / 256;
  const long b0 = (long)threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
  int64_t mine = 0;
  for (long b = b0; b < b1; ++b) mine += blkcnt[b];
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  int64_t run = base;
  for (int t = 0; t < (int)threadIdx.x; ++t) run += s_sum[t];
  for (long b = b0; b < b1; ++b) {
    offs[b] = run;
    run += blkcnt[b];
  }
  if (threadIdx.x == 255) {  // run = cnt[r] + every kept candidate of the round
    cnt[r + 1] = run < K ? run : K;
    if (r == RE_ROUNDS - 1 && run < K) atomicOr(flags, MGN_RANDEDGE_ERR_SHORT);
  }
}

__global__ void __launch_bounds__(RE_THREADS) k_re_fill(int r, long M, long K, long E, const int64_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                        const int64_t* __restrict__ offs, int64_t* __restrict__ out0,
                                                        int64_t* __restrict__ out1) {
  if (cnt[r] >= K) return;
  const long base = (long)blockIdx.x * RE_BLOCK;
  int64_t at = offs[blockIdx.x];  // slot of this workgroup's first kept candidate
  for (int p = 0; p < RE_ITEMS; ++p) {
    const long c = base + (long)p * RE_THREADS + threadIdx.x;
    const int32_t l = c < M ? lo[c] : -1;
    const bool keep = l >= 0;
    const int64_t s = block_compact_slot<RE_THREADS>(keep, p, at);
    if (keep && s < K) {  // acceptance stops at K: the output holds exactly E + 2 K columns
      const int64_t h = (int64_t)hi[c];
      out0[E + s] = (int64_t)l, out1[E + s] = h;
      out0[E + K + s] = h, out1[E + K + s] = (int64_t)l;
    }
  }
}

// ---------------------------------------------------------------------------------------- host side
struct RePlan {
  size_t header, keys, vals, lo, hi, slot, blkcnt, offs, total;
  int64_t M, cap, nb;
};

static int64_t re_pairs(int64_t N) { return N * (N - 1) / 2; }  // N < 2^31: below 2^61

extern "C" int64_t mgn_randedge_default_candidates(int64_t N, int64_t E, int64_t K) {
  if (N < 2 || N > RE_NMAX || E < 0 || E > RE_NMAX || K < 0) return 0;
  const double P = (double)re_pairs(N);
  if ((double)E >= P) return 0;
  return (int64_t)(1.1 * (double)K / (1.0 - (double)E / P)) + 64;
}

// 0 = fine, otherwise the message of the first argument that is out of range
static const char* re_plan(int64_t N, int64_t E, int64_t K, int64_t M, RePlan* p) {
  if (N < 2 || N > RE_NMAX) return "N must be in [2, 2^31 - 1]";
  if (E < 1 || E > RE_NMAX) return "E must be in [1, 2^31 - 1]";
  if (K < 1 || K > E) return "K must be in [1, E]";
  if (4 * (E + K) > re_pairs(N)) return "dense graph: 4 (E + K) must not exceed N (N - 1) / 2 (the sparse regime)";
  if (M == 0) M = mgn_randedge_default_candidates(N, E, K);
  if (M < 1 || M > RE_MMAX) return "M must be in [1, 2^30 - 1] (0 = default)";
  const int64_t need = E + K + M;  // distinct codes the table can come to hold: input pairs, accepted pairs, one cut-off round
  int64_t cap = 256;
  while (cap < need + need / 2 + 1) cap <<= 1;  // load factor <= 2/3
  if (cap > RE_CAPMAX) return "E + K + M too large for the pair table (2^31 slots)";
  WsCarver c;
  p->M = M, p->cap = cap, p->nb = (M + RE_BLOCK - 1) / RE_BLOCK;
  p->header = c.take(256);  // cnt[RE_ROUNDS + 1] int64
  p->keys = c.take((size_t)cap * 12);
  p->vals = p->keys + (size_t)cap * 8;  // directly behind the keys: one memset of all-ones bytes sets both
  p->lo = c.take((size_t)M * 4);
  p->hi = c.take((size_t)M * 4);
  p->slot = c.take((size_t)M * 4);
  p->blkcnt = c.take((size_t)p->nb * 4);
  p->offs = c.take((size_t)p->nb * 8);
  p->total = align256(c.end);
  return nullptr;
}

extern "C" size_t mgn_randedge_workspace_bytes(int64_t N, int64_t E, int64_t K, int64_t M) {
  RePlan p;
  if (re_plan(N, E, K, M, &p)) return 0;
  return p.total + 256;
}

extern "C" int mgn_randedge(const int64_t* row0, const int64_t* row1, int64_t E, int64_t N, int64_t K, int64_t M, uint64_t seed,
                            uint32_t offset, int64_t* out0, int64_t* out1, int* flags, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  RePlan p;
  if (const char* why = re_plan(N, E, K, M, &p)) return failf(1, "mgn_randedge", why);
  if (!row0 || !row1) return fail(1, "mgn_randedge: row0 / row1 must not be null");
  if (!out0 || !out1) return fail(1, "mgn_randedge: out0 / out1 must not be null");
  if (!flags) return fail(1, "mgn_randedge: flags must not be null");
  char* w = ws_base(ws, ws_bytes, p.total);
  if (!w) return fail(1, "mgn_randedge: workspace (ws_bytes) too small: see mgn_randedge_workspace_bytes");
  int64_t* cnt = (int64_t*)(w + p.header);
  unsigned long long* keys = (unsigned long long*)(w + p.keys);
  uint32_t* vals = (uint32_t*)(w + p.vals);
  int32_t *lo = (int32_t*)(w + p.lo), *hi = (int32_t*)(w + p.hi);
  uint32_t *slot = (uint32_t*)(w + p.slot), *blkcnt = (uint32_t*)(w + p.blkcnt);
  int64_t* offs = (int64_t*)(w + p.offs);
  const uint64_t mask = (uint64_t)p.cap - 1;
  const long Ml = (long)p.M;
  if (hipMemsetAsync(cnt, 0, 256, s) != hipSuccess) return fail(2, "mgn_randedge: memset");
  if (hipMemsetAsync(keys, 0xff, (size_t)p.cap * 12, s) != hipSuccess) return fail(2, "mgn_randedge: memset");
  // every slot of the new columns holds an in-range id also where the rounds come up short
  if (hipMemsetAsync(out0 + E, 0, (size_t)K * 16, s) != hipSuccess) return fail(2, "mgn_randedge: memset");
  if (hipMemsetAsync(out1 + E, 0, (size_t)K * 16, s) != hipSuccess) return fail(2, "mgn_randedge: memset");
  hipLaunchKernelGGL(k_re_input, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, row0, row1, (long)E, (long)N, out0, out1, keys, vals, mask,
                     flags);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ RE_KEY_TWEAK;
  for (int r = 0; r < RE_ROUNDS; ++r) {
    hipLaunchKernelGGL(k_re_cand, dim3((unsigned)((Ml + 255) / 256)), dim3(256), 0, s, r, Ml, (long)N, (long)K, k0, k1, offset,
                       (const int64_t*)cnt, keys, vals, mask, lo, hi, slot, flags);
    hipLaunchKernelGGL(k_re_flag, dim3((unsigned)p.nb), dim3(RE_THREADS), 0, s, r, Ml, (long)K, (const int64_t*)cnt, lo, (const uint32_t*)slot,
                       (const uint32_t*)vals, blkcnt);
    hipLaunchKernelGGL(k_re_scan, dim3(1), dim3(256), 0, s, r, (long)p.nb, (long)K, cnt, (const uint32_t*)blkcnt, offs, flags);
    hipLaunchKernelGGL(k_re_fill, dim3((unsigned)p.nb), dim3(RE_THREADS), 0, s, r, Ml, (long)K, (long)E, (const int64_t*)cnt,
                       (const int32_t*)lo, (const int32_t*)hi, (const int64_t*)offs, out0, out1);
  }
  return check_launch("mgn_randedge");
}
