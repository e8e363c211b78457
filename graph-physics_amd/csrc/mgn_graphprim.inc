// Edge primitives shared by the graph-construction units (mgn_prep, mgn_khop, mgn_subgraph, mgn_randedge); include
// mgn_host.inc first.  Two things live here: coalescing an edge list through 64-bit keys, and ordered stream compaction by a
// workgroup.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

// ---------------------------------------------------------------------------------------- edge keys
// The pair (row0, row1) of a graph on N nodes is the key row0 * N + row1 (N * N must fit 64 bits), so sorted keys are pairs
// sorted by (row0, row1).  A pair that is not to appear in the result -- an index outside [0, N), a self loop where the caller
// drops those, an unused slot -- gets the all-ones key: it sorts last, and all of them collapse into ONE trailing entry of the
// unique list, which edge_key_count() leaves out.
#define EDGE_KEY_DROPPED (~0ull)
__device__ __forceinline__ uint64_t edge_key(int64_t row0, int64_t row1, long N) {
  return (uint64_t)row0 * (uint64_t)N + (uint64_t)row1;
}

// real keys in a unique list of *n_uniq entries
__device__ __forceinline__ size_t edge_key_count(const uint64_t* __restrict__ uniq, const size_t* __restrict__ n_uniq) {
  size_t n = *n_uniq;
  if (n > 0 && uniq[n - 1] == EDGE_KEY_DROPPED) --n;
  return n;
}

// Edge list -> keys; an index outside [0, N) sets *err and drops the edge.
//   BOTH   keys[e] = (row0, row1) and keys[E + e] = (row1, row0): to_undirected before coalescing, self loops stay
//   !BOTH  keys[e] = (row0, row1), a self loop is dropped
template <bool BOTH>
__global__ void __launch_bounds__(256) k_edge_list_keys(const int64_t* __restrict__ row0, const int64_t* __restrict__ row1, long E, long N,
                                                        uint64_t* __restrict__ keys, int* __restrict__ err) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t a = row0[e], b = row1[e];
  const bool ok = a >= 0 && a < N && b >= 0 && b < N;
  if (!ok) *err = 1;
  if (BOTH) {
    keys[e] = ok ? edge_key(a, b, N) : EDGE_KEY_DROPPED;
    keys[E + e] = ok ? edge_key(b, a, N) : EDGE_KEY_DROPPED;
  } else {
    keys[e] = (ok && a != b) ? edge_key(a, b, N) : EDGE_KEY_DROPPED;
  }
}

// The two host functions are templates (Key is always uint64_t) so that a unit which only compacts does not instantiate, and
// ship, rocPRIM's sort kernels.
// rocPRIM temporary bytes sort_unique_keys needs for n keys
template <class Key = uint64_t>
static size_t sort_unique_tmp_bytes(size_t n) {
  size_t t1 = 0, t2 = 0;
  (void)rocprim::radix_sort_keys(nullptr, t1, (Key*)nullptr, (Key*)nullptr, n, 0, 64, (hipStream_t)0);
  (void)rocprim::unique(nullptr, t2, (Key*)nullptr, (Key*)nullptr, (size_t*)nullptr, n, rocprim::equal_to<Key>(), (hipStream_t)0);
  return (t1 > t2 ? t1 : t2) + 256;
}

// keys[n] -> sorted[n] -> uniq[*n_uniq] (ascending, distinct; *n_uniq on the device); `who` prefixes the message of a failure
template <class Key>
static int sort_unique_keys(void* tmp, size_t tmp_bytes, Key* keys, Key* sorted, Key* uniq, size_t* n_uniq, size_t n, hipStream_t s,
                            const char* who) {
  static_assert(sizeof(Key) == 8, "edge keys are 64-bit");
  size_t tb = tmp_bytes;
  if (rocprim::radix_sort_keys(tmp, tb, keys, sorted, n, 0, 64, s) != hipSuccess) return failf(2, who, "sort");
  tb = tmp_bytes;
  if (rocprim::unique(tmp, tb, sorted, uniq, n_uniq, n, rocprim::equal_to<Key>(), s) != hipSuccess) return failf(2, who, "unique");
  return 0;
}

// ---------------------------------------------------------------------------------------- ordered stream compaction
// A workgroup of THREADS threads (whole wave64s) walks its items in passes: thread t of pass p looks at item
// block * THREADS * passes + p * THREADS + t, so a wave reads 64 consecutive items.  A flag kernel counts the kept items of
// every workgroup, an exclusive scan of the counts gives each workgroup the slot of its first kept item, and a fill kernel
// places kept item i at that slot + the kept items before i: input order survives, no global atomics, bit-identical from
// run to run.  Every thread of the workgroup calls these (ballots and barriers), kept or not.

// kept items of this wave in one pass (wave-uniform)
__device__ __forceinline__ unsigned wave_kept(bool keep) { return (unsigned)__popcll(__ballot(keep)); }

// sum over the workgroup of each wave's count, delivered to thread 0
template <int THREADS>
__device__ __forceinline__ unsigned block_kept(unsigned wave_count) {
  __shared__ unsigned s_cnt[THREADS / 64];
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = wave_count;
  __syncthreads();
  unsigned c = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < THREADS / 64; ++w) c += s_cnt[w];
  return c;
}

// slot of this thread's item in pass p if it is kept: base + the kept items of lower waves + of lower lanes; then base moves on
// by the pass's total.  wave64 __ballot / popcount ranks and a cross-wave scan of the wave counts in LDS, double-buffered on
// p & 1 so that one barrier per pass is enough.
template <int THREADS>
__device__ __forceinline__ int64_t block_compact_slot(bool keep, int p, int64_t& base) {
  __shared__ unsigned s_cnt[2][THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long votes = __ballot(keep);
  const unsigned rank = (unsigned)__popcll(votes & ((1ull << lane) - 1ull));
  if (lane == 0) s_cnt[p & 1][wave] = (unsigned)__popcll(votes);
  __syncthreads();
  unsigned before = 0, total = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    const unsigned c = s_cnt[p & 1][w];
    if (w < wave) before += c;
    total += c;
  }
  const int64_t slot = base + before + rank;
  base += total;
  return slot;
}
