// MI355X (gfx950) k-hop edge sets: all ordered pairs (i, j), i != j, joined by a directed walk of 1..k edges -- what the
// reference builds per trajectory on the CPU by repeated sparse products (graphphysics/utils/torch_graph.py:14-105,
// dataset/dataset.py:206-242, the config key dataset.khop).  Integer-only, deterministic, sorted by (row0, row1) like a
// coalesced COO tensor.  Sixth translation unit of libmgn_hip.so; sort / unique / select / scan are rocPRIM (header-only).
//
//   prep      key = row0 * N + row1 -> radix sort -> unique -> CSR of the adjacency (rowptr int64 [N+1], col int32)
//   row       one wavefront per origin row: breadth-first search over the CSR with an open-addressing hash set and the
//             list of inserted ids (= the BFS queue) in LDS.  Instantiated as COUNT (row size, or the overflow mark when
//             the row outgrows KH_CAP ids) and FILL (search again, bitonic sort of the ids in LDS, int64 stores at the
//             row's offset = exclusive scan of the counts).
//   overflow  rows above KH_CAP (hub nodes, large k on 3-D meshes): one workgroup per row, three bitmaps of N bits in the
//             caller's workspace (visited / frontier / next), level-synchronous with atomicOr; count = popcount, fill =
//             ordered scan with prefix popcounts.  KH_BATCH rows are in flight at a time (a persistent grid), so the
//             workspace is bounded.  Exact but slow: ~3 * N/32 words per level per row.
// No global atomics on the fill path of either kind: the output is bit-identical run to run.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include "mgn_hip.h"
#include "mgn_host.inc"       // g_err, fail, check_launch, workspace carving, count -> fill header
#include "mgn_graphprim.inc"  // edge keys, sort_unique_keys

extern "C" const char* mgn_khop_last_error(void) { return g_err; }

#define KH_CAP 1024            // ids one row may hold on the LDS path (a power of two: the bitonic sort pads to it)
#define KH_SLOTS (2 * KH_CAP)  // hash slots per row: the set stays at most half full, so probing ends
#define KH_WAVES 4             // rows (= waves) per workgroup: 4 * (8 KB set + 4 KB list) = 48 KB of LDS
#define KH_BATCH 128           // overflow rows in flight (3 bitmaps of N bits each)
#define KH_EMPTY 0xffffffffu
#define KH_NMAX 2147483646LL   // node ids are 32-bit in LDS and all-ones is the empty slot
#define KH_MAGIC 0x6b686f70313336ull

// ---------------------------------------------------------------------------------------- prep: edge list -> CSR
// keys by k_edge_list_keys<false>: one direction, and self loops are dropped -- they carry nothing (the origin never appears
// in its own row).
__global__ void __launch_bounds__(256) k_khop_col(const uint64_t* __restrict__ uniq, const size_t* __restrict__ n_uniq, long N, long E,
                                                  int32_t* __restrict__ col) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E || (size_t)i >= edge_key_count(uniq, n_uniq)) return;
  col[i] = (int32_t)(uniq[i] % (uint64_t)N);
}

// rowptr[r] = first position whose key is >= r * N (r = 0..N): a binary search per row, no imbalance on isolated runs
__global__ void __launch_bounds__(256) k_khop_rowptr(const uint64_t* __restrict__ uniq, const size_t* __restrict__ n_uniq, long N,
                                                     int64_t* __restrict__ rowptr) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > N) return;
  const size_t n = edge_key_count(uniq, n_uniq);
  const uint64_t want = (uint64_t)r * (uint64_t)N;
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (uniq[mid] < want) lo = mid + 1; else hi = mid;
  }
  rowptr[r] = (int64_t)lo;
}

// ---------------------------------------------------------------------------------------- row kernel (LDS path)
// LDS writes of one phase are made visible to every lane of the wave before the next phase reads them: a workgroup-scope
// fence (drains the LDS queue) and a wave barrier (no lane runs ahead); nothing relies on lockstep.
__device__ __forceinline__ void khop_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

struct KhopRow {
  unsigned* set;   // [KH_SLOTS]
  unsigned* list;  // [KH_CAP] ids in insertion order = the BFS queue
  unsigned* n;     // ids inserted so far (may run past KH_CAP: those are counted, not stored)
};

__device__ __forceinline__ void khop_insert(const KhopRow& R, unsigned origin, unsigned v) {
  if (v == origin) return;
  // stop feeding a row that has overflowed: every lane can pass this test at most once with a stale count, so the set never
  // holds more than KH_CAP + 64 of its 2 * KH_CAP slots and the probe below always meets an empty slot or the id itself
  if (__hip_atomic_load(R.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > KH_CAP) return;
  unsigned h = (v * 2654435761u) >> 21;  // 32 - log2(KH_SLOTS)
  for (int probe = 0; probe < KH_SLOTS; ++probe) {
    const unsigned old = atomicCAS(&R.set[h], KH_EMPTY, v);
    if (old == v) return;
    if (old == KH_EMPTY) {
      const unsigned at = atomicAdd(R.n, 1u);
      if (at < KH_CAP) R.list[at] = v;  // past the capacity: dropped, the count marks the row
      return;
    }
    h = (h + 1) & (KH_SLOTS - 1);
  }
}
static_assert(KH_SLOTS == 2048, "the hash shift in khop_insert is 32 - log2(KH_SLOTS)");

template <bool FILL>
__global__ void __launch_bounds__(64 * KH_WAVES) k_khop_rows(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, long N,
                                                            int hops, int64_t* __restrict__ cnt, const int64_t* __restrict__ offs,
                                                            int64_t* __restrict__ out0, int64_t* __restrict__ out1) {
  __shared__ __attribute__((aligned(16))) unsigned s_set[KH_WAVES][KH_SLOTS];
  __shared__ __attribute__((aligned(16))) unsigned s_list[KH_WAVES][KH_CAP];
  __shared__ unsigned s_n[KH_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * KH_WAVES + wave;
  if (row >= N) return;  // wave-uniform; the kernel has no workgroup barrier
  if (FILL && (cnt[row] == 0 || cnt[row] > KH_CAP)) return;  // nothing to write / written by the overflow path
  KhopRow R{s_set[wave], s_list[wave], &s_n[wave]};
  uint4* set4 = (uint4*)R.set;
  for (int i = lane; i < KH_SLOTS / 4; i += 64) set4[i] = make_uint4(KH_EMPTY, KH_EMPTY, KH_EMPTY, KH_EMPTY);
  if (lane == 0) *R.n = 0;
  khop_wave_sync();

  const unsigned origin = (unsigned)row;
  // level 1: the origin's own row, one edge per lane
  for (int64_t e = rowptr[row] + lane, end = rowptr[row + 1]; e < end; e += 64) khop_insert(R, origin, (unsigned)col[e]);
  khop_wave_sync();
  // levels 2..hops: the ids of the previous level are list[lo, hi); eight lanes share one frontier entry.  hi is a snapshot:
  // the list grows while the level is expanded, and what it gains belongs to the next level.
  unsigned lo = 0;
  const int grp = lane >> 3, sub = lane & 7;
  for (int lvl = 1; lvl < hops; ++lvl) {
    const unsigned n_now = __builtin_amdgcn_readfirstlane(__hip_atomic_load(R.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (n_now > KH_CAP || n_now == lo) break;  // overflowed, or the search has closed
    const unsigned hi = n_now;
    for (unsigned f = lo + grp; f < hi; f += 8) {
      const unsigned v = R.list[f];
      for (int64_t e = rowptr[v] + sub, end = rowptr[v + 1]; e < end; e += 8) khop_insert(R, origin, (unsigned)col[e]);
    }
    lo = hi;
    khop_wave_sync();
  }
  const unsigned n = __builtin_amdgcn_readfirstlane(__hip_atomic_load(R.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  if (!FILL) {
    if (lane == 0) cnt[row] = n > KH_CAP ? -1 : (int64_t)n;
    return;
  }
  if (n > KH_CAP) return;  // cannot happen after a count that said otherwise; never write past the row
  // ascending ids: bitonic network over the list padded with all-ones to a power of two P (64 <= P <= KH_CAP)
  unsigned P = 64;
  while (P < n) P <<= 1;
  for (unsigned i = n + lane; i < P; i += 64) R.list[i] = KH_EMPTY;
  khop_wave_sync();
  for (unsigned k = 2; k <= P; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned t = lane; t < P / 2; t += 64) {
        const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // the lower index of pair t: bit j clear
        const unsigned p = i | j;
        const unsigned a = R.list[i], b = R.list[p];
        const bool up = (i & k) == 0;
        if ((a > b) == up) {
          R.list[i] = b;
          R.list[p] = a;
        }
      }
      khop_wave_sync();
    }
  const int64_t off = offs[row], room = offs[row + 1] - off;  // room == n: the search is deterministic; never write past the row
  for (unsigned i = lane; i < n && (int64_t)i < room; i += 64) {
    out0[off + i] = (int64_t)row;
    out1[off + i] = (int64_t)R.list[i];
  }
}

// ---------------------------------------------------------------------------------------- overflow rows (bitmap path)
// The bitmaps live in global memory and are shared by the threads of one workgroup only.  Every access is an agent-scope
// atomic (served by the L2, never by a CU's vector cache line that an atomicOr has gone past), phases are separated by
// __threadfence() + __syncthreads().
__device__ __forceinline__ unsigned bm_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void bm_st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void bm_sync() {
  __threadfence();
  __syncthreads();
}

struct IsOverflow {
  const int64_t* cnt;
  __device__ bool operator()(const int32_t& r) const { return cnt[r] < 0; }
};

template <bool FILL>
__global__ void __launch_bounds__(256) k_khop_overflow(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, long N, int hops,
                                                       const int32_t* __restrict__ ovf, const size_t* __restrict__ n_ovf,
                                                       unsigned* __restrict__ bitmaps, int64_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ offs, int64_t* __restrict__ out0,
                                                       int64_t* __restrict__ out1) {
  __shared__ unsigned s_red[4];
  __shared__ unsigned s_any;
  const long W = (N + 31) >> 5;
  unsigned* visited = bitmaps + (size_t)blockIdx.x * 3 * (size_t)W;
  unsigned* cur = visited + W;
  unsigned* nxt = cur + W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t rows = *n_ovf;
  for (size_t it = blockIdx.x; it < rows; it += gridDim.x) {
    const long origin = ovf[it];
    for (long w = tid; w < W; w += 256) {
      const unsigned bit = (w == (origin >> 5)) ? (1u << (origin & 31)) : 0u;
      bm_st(&visited[w], bit);
      bm_st(&cur[w], bit);
      bm_st(&nxt[w], 0u);
    }
    bm_sync();
    for (int lvl = 0; lvl < hops; ++lvl) {
      if (tid == 0) s_any = 0;
      __syncthreads();
      for (long w = tid; w < W; w += 256) {
        unsigned bits = bm_ld(&cur[w]);
        while (bits) {
          const int b = __ffs((int)bits) - 1;
          bits &= bits - 1;
          const long v = (w << 5) + b;
          for (int64_t e = rowptr[v], end = rowptr[v + 1]; e < end; ++e) {
            const unsigned u = (unsigned)col[e], m = 1u << (u & 31);
            if (!(bm_ld(&visited[u >> 5]) & m)) atomicOr(&nxt[u >> 5], m);
          }
        }
      }
      bm_sync();
      unsigned any = 0;
      for (long w = tid; w < W; w += 256) {  // word w belongs to one thread here: plain read-modify-write
        const unsigned seen = bm_ld(&visited[w]);
        const unsigned fresh = bm_ld(&nxt[w]) & ~seen;
        bm_st(&visited[w], seen | fresh);
        bm_st(&cur[w], fresh);
        bm_st(&nxt[w], 0u);
        any |= fresh;
      }
      if (any) s_any = 1;  // every writer stores 1
      bm_sync();
      const unsigned go = s_any;
      __syncthreads();  // everyone has read it before thread 0 resets it for the next level
      if (!go) break;   // uniform
    }
    // the origin is not part of its own row
    if (tid == 0) bm_st(&visited[origin >> 5], bm_ld(&visited[origin >> 5]) & ~(1u << (origin & 31)));
    bm_sync();
    if (!FILL) {
      unsigned c = 0;
      for (long w = tid; w < W; w += 256) c += __popc(bm_ld(&visited[w]));
      for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
      if (lane == 0) s_red[wave] = c;
      __syncthreads();
      if (tid == 0) cnt[origin] = (int64_t)s_red[0] + s_red[1] + s_red[2] + s_red[3];
      __syncthreads();
    } else {
      // ascending by construction: tiles of 256 words in order, an exclusive prefix popcount inside the tile
      int64_t base = offs[origin];
      const int64_t stop = offs[origin + 1];  // == base + popcount; never write past the row
      for (long w0 = 0; w0 < W; w0 += 256) {
        const long w = w0 + tid;
        unsigned bits = w < W ? bm_ld(&visited[w]) : 0u;
        const unsigned c = __popc(bits);
        unsigned incl = c;
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        if (lane == 63) s_red[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int q = 0; q < 4; ++q) {
          if (q < wave) before += s_red[q];
          total += s_red[q];
        }
        int64_t at = base + before + (incl - c);
        while (bits && at < stop) {
          const int b = __ffs((int)bits) - 1;
          bits &= bits - 1;
          out0[at] = (int64_t)origin;
          out1[at] = (int64_t)((w << 5) + b);
          ++at;
        }
        base += total;
        __syncthreads();
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- host side
struct KhopHeader {  // first 256 bytes of the workspace: what mgn_khop_fill needs from mgn_khop_count
  uint64_t magic;
  int64_t N, E, hops, n_out, n_overflow;
};

struct KhopPlan {
  size_t header, keys, sorted, uniq, flags, rowptr, col, cnt, offs, ovf, bitmaps, tmp, tmp_bytes, total;
};
static KhopPlan khop_plan(int64_t N, int64_t E) {
  KhopPlan p;
  WsCarver c;
  const size_t n = (size_t)E, rows = (size_t)N;
  size_t t3 = 0, t4 = 0;  // the temporary block serves sort + unique, select and scan in turn
  (void)rocprim::select(nullptr, t3, rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, (size_t*)nullptr, rows, IsOverflow{nullptr}, (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, t4, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, rows + 1, rocprim::plus<int64_t>(), (hipStream_t)0);
  const size_t t = (t3 > t4 ? t3 : t4) + 256, tsu = sort_unique_tmp_bytes(n);
  p.tmp_bytes = t > tsu ? t : tsu;
  p.header = c.take(256);
  p.keys = c.take(n * 8);
  p.sorted = c.take(n * 8);
  p.uniq = c.take(n * 8);
  p.flags = c.take(256);  // [0] unique count (size_t), [1] overflow rows (size_t), [2] err (int)
  p.rowptr = c.take((rows + 1) * 8);
  p.col = c.take(n * 4);
  p.cnt = c.take((rows + 1) * 8);
  p.offs = c.take((rows + 1) * 8);
  p.ovf = c.take(rows * 4);
  p.bitmaps = c.take((size_t)KH_BATCH * 3 * ((rows + 31) / 32) * 4);
  p.tmp = c.take(p.tmp_bytes);
  p.total = c.end;
  return p;
}

extern "C" int mgn_khop_row_capacity(void) { return KH_CAP; }

extern "C" size_t mgn_khop_workspace_bytes(int64_t N, int64_t E) {
  if (N < 1 || N > KH_NMAX || E < 0) return 0;
  return khop_plan(N, E).total + 256;
}

extern "C" int mgn_khop_count(const int64_t* row0, const int64_t* row1, int64_t E, int64_t N, int hops, int64_t* n_out_host,
                              int64_t* n_overflow_rows_host, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hops < 2) return fail(1, "mgn_khop_count: hops must be >= 2 (one hop is the input itself)");
  if (N < 1 || N > KH_NMAX) return fail(1, "mgn_khop_count: N must be in [1, 2^31 - 2] (32-bit node ids, all-ones is the empty slot)");
  if (E < 0) return fail(1, "mgn_khop_count: E must be >= 0");
  if (!n_out_host || !n_overflow_rows_host) return fail(1, "mgn_khop_count: n_out_host / n_overflow_rows_host must not be null");
  const KhopPlan p = khop_plan(N, E);
  char* w = ws_base(ws, ws_bytes, p.total);
  if (!w) return fail(1, "mgn_khop_count: workspace (ws_bytes) too small: see mgn_khop_workspace_bytes");
  uint64_t *keys = (uint64_t*)(w + p.keys), *sorted = (uint64_t*)(w + p.sorted), *uniq = (uint64_t*)(w + p.uniq);
  size_t* n_uniq = (size_t*)(w + p.flags);
  size_t* n_ovf = n_uniq + 1;
  int* err = (int*)(n_uniq + 2);
  int64_t *rowptr = (int64_t*)(w + p.rowptr), *cnt = (int64_t*)(w + p.cnt), *offs = (int64_t*)(w + p.offs);
  int32_t *col = (int32_t*)(w + p.col), *ovf = (int32_t*)(w + p.ovf);
  unsigned* bitmaps = (unsigned*)(w + p.bitmaps);
  KhopHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = KH_MAGIC; h.N = N; h.E = E; h.hops = hops;
  *n_out_host = 0;
  *n_overflow_rows_host = 0;
  if (int rc = ws_header_clear(w + p.header, 256, s, "mgn_khop_count")) return rc;
  if (hipMemsetAsync(w + p.flags, 0, 256, s) != hipSuccess) return fail(2, "mgn_khop_count: memset");
  if (E > 0) {
    hipLaunchKernelGGL(k_edge_list_keys<false>, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, row0, row1, (long)E, (long)N, keys, err);
    if (int rc = sort_unique_keys(w + p.tmp, p.tmp_bytes, keys, sorted, uniq, n_uniq, (size_t)E, s, "mgn_khop_count")) return rc;
    hipLaunchKernelGGL(k_khop_col, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, uniq, n_uniq, (long)N, (long)E, col);
  }
  // with E == 0 the unique count stays 0 and every rowptr entry is 0
  hipLaunchKernelGGL(k_khop_rowptr, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, uniq, n_uniq, (long)N, rowptr);
  if (hipMemsetAsync(cnt + N, 0, sizeof(int64_t), s) != hipSuccess) return fail(2, "mgn_khop_count: memset");
  const unsigned row_grid = (unsigned)((N + KH_WAVES - 1) / KH_WAVES);
  hipLaunchKernelGGL(k_khop_rows<false>, dim3(row_grid), dim3(64 * KH_WAVES), 0, s, rowptr, col, (long)N, hops, cnt, (const int64_t*)nullptr,
                     (int64_t*)nullptr, (int64_t*)nullptr);
  size_t tb = p.tmp_bytes;
  if (rocprim::select(w + p.tmp, tb, rocprim::counting_iterator<int32_t>(0), ovf, n_ovf, (size_t)N, IsOverflow{cnt}, s) != hipSuccess)
    return fail(2, "mgn_khop_count: select");
  hipLaunchKernelGGL(k_khop_overflow<false>, dim3(KH_BATCH), dim3(256), 0, s, rowptr, col, (long)N, hops, ovf, n_ovf, bitmaps, cnt,
                     (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
  tb = p.tmp_bytes;
  if (rocprim::exclusive_scan(w + p.tmp, tb, cnt, offs, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), s) != hipSuccess)
    return fail(2, "mgn_khop_count: scan");
  if (int rc = check_launch("mgn_khop_count")) return rc;
  int64_t total = 0;
  unsigned long long flags[3] = {0, 0, 0};
  if (hipMemcpyAsync(&total, offs + N, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(2, "mgn_khop_count: memcpy");
  if (hipMemcpyAsync(flags, w + p.flags, sizeof(flags), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(2, "mgn_khop_count: memcpy");
  if (hipStreamSynchronize(s) != hipSuccess) return fail(2, "mgn_khop_count: sync failed");
  if (*(int*)&flags[2]) return fail(3, "mgn_khop_count: edge index outside [0, N)");
  h.n_out = total;
  h.n_overflow = (int64_t)flags[1];
  if (int rc = ws_header_put(w + p.header, &h, sizeof(h), s, "mgn_khop_count")) return rc;
  *n_out_host = total;
  *n_overflow_rows_host = h.n_overflow;
  return 0;
}

extern "C" int mgn_khop_fill(const void* ws, size_t ws_bytes, int64_t N, int hops, int64_t* out0, int64_t* out1, int64_t cap, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hops < 2) return fail(1, "mgn_khop_fill: hops must be >= 2");
  if (N < 1 || N > KH_NMAX) return fail(1, "mgn_khop_fill: N must be in [1, 2^31 - 2]");
  if (!ws || ws_bytes < 512) return fail(1, "mgn_khop_fill: workspace (ws_bytes) too small");
  if (cap < 0) return fail(1, "mgn_khop_fill: cap must be >= 0");
  char* w = (char*)align256((size_t)ws);  // the header fits: 255 + 256 < 512
  KhopHeader h;
  if (int rc = ws_header_get(w, &h, sizeof(h), s, "mgn_khop_fill")) return rc;
  if (h.magic != KH_MAGIC || h.N != N || h.hops != hops) return fail(1, "mgn_khop_fill: the workspace does not hold a mgn_khop_count of this N / hops");
  const KhopPlan p = khop_plan(N, h.E);
  if (!ws_base(ws, ws_bytes, p.total)) return fail(1, "mgn_khop_fill: workspace (ws_bytes) too small");
  if (cap < h.n_out) return fail(1, "mgn_khop_fill: cap is smaller than the counted number of pairs");
  if (h.n_out == 0) return 0;
  if (!out0 || !out1) return fail(1, "mgn_khop_fill: out0 / out1 must not be null");
  const int64_t *rowptr = (const int64_t*)(w + p.rowptr), *offs = (const int64_t*)(w + p.offs);
  int64_t* cnt = (int64_t*)(w + p.cnt);
  const int32_t *col = (const int32_t*)(w + p.col), *ovf = (const int32_t*)(w + p.ovf);
  const size_t* n_ovf = (const size_t*)(w + p.flags) + 1;
  unsigned* bitmaps = (unsigned*)(w + p.bitmaps);
  const unsigned row_grid = (unsigned)((N + KH_WAVES - 1) / KH_WAVES);
  hipLaunchKernelGGL(k_khop_rows<true>, dim3(row_grid), dim3(64 * KH_WAVES), 0, s, rowptr, col, (long)N, hops, cnt, offs, out0, out1);
  if (h.n_overflow > 0)
    hipLaunchKernelGGL(k_khop_overflow<true>, dim3(KH_BATCH), dim3(256), 0, s, rowptr, col, (long)N, hops, ovf, n_ovf, bitmaps, cnt, offs, out0, out1);
  return check_launch("mgn_khop_fill");
}
