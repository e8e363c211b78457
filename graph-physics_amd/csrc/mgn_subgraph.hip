// MI355X (gfx950) induced sub-meshes: what the reference's Dataset does per sample when it trains a mesh in parts
// (graphphysics/dataset/dataset.py:244-327, torch_geometric.utils.subgraph(..., relabel_nodes=True) of torch-geometric 2.6.1):
// keep the edges whose two ends are in a node subset, in input order, relabelled to the position in the subset; cut edges are
// dropped.  Integer work and row copies only.  Seventh translation unit of libmgn_hip.so; the scan of the per-workgroup counts
// is rocPRIM (header-only).
//
//   table   new_index[N] int32 = -1 (a memset of all-ones bytes); new_index[node_ids[i]] = i; a second pass over the subset
//           checks new_index[node_ids[i]] == i: of two entries that name one node only one can own the slot, so a repeated id
//           is found in O(S), whichever store won.
//   flag    one workgroup per SG_BLOCK consecutive edges: relabel both ends through the table, keep = both >= 0; the relabelled
//           pair goes to the workspace as two int32 (-1 in the first marks a dropped edge), the workgroup's number of kept edges
//           to cnt[block].  Exclusive scan of cnt -> offs; offs[blocks] = E'.
//   fill    the same workgroups over the int32 pairs (8 bytes per edge instead of 16 + two table lookups).  Output slot =
//           offs[block] + rank: the ordered stream compaction of mgn_graphprim.inc, no global atomics, bit-identical from
//           run to run.
//   gather  mgn_gather_rows_batch: dst[r, :width] = src[idx[r], :width] for up to 8 jobs in one launch -- the per-frame work
//           of a cached part (x, y, pos rows by node id, edge_attr rows by edge position).
#include <rocprim/device/device_scan.hpp>
#include "mgn_hip.h"
#include "mgn_host.inc"       // g_err, fail, check_launch, workspace carving, count -> fill header
#include "mgn_graphprim.inc"  // wave_kept, block_kept, block_compact_slot

extern "C" const char* mgn_subgraph_last_error(void) { return g_err; }

#define SG_THREADS 256
#define SG_ITEMS 8
#define SG_BLOCK (SG_THREADS * SG_ITEMS)  // edges one workgroup compacts
#define SG_NMAX 2147483646LL              // node ids and subset positions are int32 in the table
#define SG_EMAX (1LL << 40)               // blocks = E / SG_BLOCK stays far below the grid limit
#define SG_MAGIC 0x7375626731333600ull
#define SG_ERR_RANGE 1
#define SG_ERR_DUP 2

// ---------------------------------------------------------------------------------------- relabel table
__global__ void __launch_bounds__(256) k_sg_table_set(const int64_t* __restrict__ ids, long S, long N, int32_t* __restrict__ table,
                                                      int* __restrict__ err) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const int64_t v = ids[i];
  if (v < 0 || v >= N) {
    atomicOr(err, SG_ERR_RANGE);
    return;
  }
  table[v] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_sg_table_check(const int64_t* __restrict__ ids, long S, long N, const int32_t* __restrict__ table,
                                                        int* __restrict__ err) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const int64_t v = ids[i];
  if (v < 0 || v >= N) return;  // reported by k_sg_table_set
  if (table[v] != (int32_t)i) atomicOr(err, SG_ERR_DUP);
}

// ---------------------------------------------------------------------------------------- flag + count
// thread t of pass p looks at edge block * SG_BLOCK + p * SG_THREADS + t: a wave reads 64 consecutive edges
__global__ void __launch_bounds__(SG_THREADS) k_sg_flag(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, long E, long N,
                                                        const int32_t* __restrict__ table, int32_t* __restrict__ ls,
                                                        int32_t* __restrict__ ld, int64_t* __restrict__ cnt, int* __restrict__ err) {
  const long base = (long)blockIdx.x * SG_BLOCK;
  unsigned kept = 0;  // wave-uniform
  for (int p = 0; p < SG_ITEMS; ++p) {
    const long e = base + (long)p * SG_THREADS + threadIdx.x;
    bool keep = false;
    if (e < E) {
      const int64_t a = src[e], b = dst[e];
      int32_t la = -1, lb = -1;
      if (a >= 0 && a < N && b >= 0 && b < N) {
        la = table[a];
        lb = table[b];
      } else {
        atomicOr(err, SG_ERR_RANGE);
      }
      keep = la >= 0 && lb >= 0;
      ls[e] = keep ? la : -1;
      ld[e] = lb;
    }
    kept += wave_kept(keep);
  }
  const unsigned c = block_kept<SG_THREADS>(kept);
  if (threadIdx.x == 0) cnt[blockIdx.x] = (int64_t)c;
}

// ---------------------------------------------------------------------------------------- fill (ordered compaction)
__global__ void __launch_bounds__(SG_THREADS) k_sg_fill(const int32_t* __restrict__ ls, const int32_t* __restrict__ ld, long E,
                                                        const int64_t* __restrict__ offs, long n_out, int64_t* __restrict__ out_src,
                                                        int64_t* __restrict__ out_dst, int64_t* __restrict__ out_pos,
                                                        uint8_t* __restrict__ out_mask) {
  const long base = (long)blockIdx.x * SG_BLOCK;
  int64_t at = offs[blockIdx.x];  // slot of this workgroup's first kept edge
  for (int p = 0; p < SG_ITEMS; ++p) {
    const long e = base + (long)p * SG_THREADS + threadIdx.x;
    const int32_t a = e < E ? ls[e] : -1;
    const bool keep = a >= 0;
    const int64_t slot = block_compact_slot<SG_THREADS>(keep, p, at);
    if (keep && slot < n_out) {  // == by construction; never write past the counted size
      out_src[slot] = (int64_t)a;
      out_dst[slot] = (int64_t)ld[e];
      out_pos[slot] = (int64_t)e;
    }
    if (out_mask && e < E) out_mask[e] = keep ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------- batched row gather
struct SgGatherArgs {
  mgn_gather_job job[MGN_MAX_GATHER_JOBS];
  int64_t tile_rows[MGN_MAX_GATHER_JOBS];       // rows one workgroup copies
  int64_t tile_start[MGN_MAX_GATHER_JOBS + 1];  // first workgroup of each job
  int n;
};

#define SG_GATHER_ROWS 1024   // index entries staged in LDS
#define SG_GATHER_ELEMS 4096  // elements one workgroup aims at

// one workgroup copies tile_rows consecutive output rows of one job; consecutive threads write consecutive elements of dst
__global__ void __launch_bounds__(256) k_sg_gather(const SgGatherArgs A) {
  __shared__ int64_t s_idx[SG_GATHER_ROWS];
  int j = 0;
  while (j + 1 < A.n && (int64_t)blockIdx.x >= A.tile_start[j + 1]) ++j;
  const mgn_gather_job J = A.job[j];
  const int64_t r0 = ((int64_t)blockIdx.x - A.tile_start[j]) * A.tile_rows[j];
  const unsigned rows = (unsigned)(J.rows - r0 < A.tile_rows[j] ? J.rows - r0 : A.tile_rows[j]);
  for (unsigned r = threadIdx.x; r < rows; r += 256) {
    const int64_t s = J.idx[r0 + r];
    s_idx[r] = (s >= 0 && s < J.src_rows) ? s : -1;  // an index outside the source is not followed
  }
  __syncthreads();
  const unsigned w = (unsigned)J.width;
  const unsigned n = rows * w;  // <= max(SG_GATHER_ELEMS, width) < 2^31
  for (unsigned i = threadIdx.x; i < n; i += 256) {
    const unsigned r = i / w, c = i - r * w;
    const int64_t s = s_idx[r];
    if (s >= 0) J.dst[(r0 + r) * J.ld_dst + c] = J.src[s * J.ld_src + c];
  }
}

// ---------------------------------------------------------------------------------------- host side
struct SgHeader {  // first 256 bytes of the workspace: what mgn_subgraph_fill needs from mgn_subgraph_count
  uint64_t magic;
  int64_t N, E, S, n_edges;
};

struct SgPlan {
  size_t header, flags, table, ls, ld, cnt, offs, tmp, tmp_bytes, total;
  int64_t blocks;
};
static SgPlan sg_plan(int64_t N, int64_t E) {
  SgPlan p;
  p.blocks = (E + SG_BLOCK - 1) / SG_BLOCK;
  const size_t nb = (size_t)p.blocks + 1;
  size_t t = 0;
  (void)rocprim::exclusive_scan(nullptr, t, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, nb, rocprim::plus<int64_t>(), (hipStream_t)0);
  p.tmp_bytes = t + 256;
  WsCarver c;
  p.header = c.take(256);
  p.flags = c.take(256);  // [0] err bits (int); directly behind the header: one memset clears both
  p.table = c.take((size_t)N * 4);
  p.ls = c.take((size_t)E * 4);
  p.ld = c.take((size_t)E * 4);
  p.cnt = c.take(nb * 8);
  p.offs = c.take(nb * 8);
  p.tmp = c.take(p.tmp_bytes);
  p.total = c.end;
  return p;
}

extern "C" int mgn_subgraph_block_edges(void) { return SG_BLOCK; }

extern "C" size_t mgn_subgraph_workspace_bytes(int64_t N, int64_t E) {
  if (N < 0 || N > SG_NMAX || E < 0 || E > SG_EMAX) return 0;
  return sg_plan(N, E).total + 256;
}

extern "C" int mgn_subgraph_count(const int64_t* node_ids, int64_t S, int64_t N, const int64_t* src, const int64_t* dst, int64_t E,
                                  int64_t* n_edges_host, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (N < 0 || N > SG_NMAX) return fail(1, "mgn_subgraph_count: N must be in [0, 2^31 - 2] (the relabel table holds 32-bit positions)");
  if (S < 0 || S > SG_NMAX) return fail(1, "mgn_subgraph_count: S must be in [0, 2^31 - 2]");
  if (E < 0 || E > SG_EMAX) return fail(1, "mgn_subgraph_count: E must be in [0, 2^40]");
  if (S > 0 && !node_ids) return fail(1, "mgn_subgraph_count: node_ids must not be null when S > 0");
  if (E > 0 && (!src || !dst)) return fail(1, "mgn_subgraph_count: src / dst must not be null when E > 0");
  if (!n_edges_host) return fail(1, "mgn_subgraph_count: n_edges_host must not be null");
  const SgPlan p = sg_plan(N, E);
  char* w = ws_base(ws, ws_bytes, p.total);
  if (!w) return fail(1, "mgn_subgraph_count: workspace (ws_bytes) too small: see mgn_subgraph_workspace_bytes");
  int* err = (int*)(w + p.flags);
  int32_t *table = (int32_t*)(w + p.table), *ls = (int32_t*)(w + p.ls), *ld = (int32_t*)(w + p.ld);
  int64_t *cnt = (int64_t*)(w + p.cnt), *offs = (int64_t*)(w + p.offs);
  *n_edges_host = 0;
  if (int rc = ws_header_clear(w + p.header, 512, s, "mgn_subgraph_count")) return rc;  // the header and the flags behind it
  if (N > 0 && hipMemsetAsync(table, 0xff, (size_t)N * 4, s) != hipSuccess) return fail(2, "mgn_subgraph_count: memset");
  if (S > 0) {
    const unsigned g = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(k_sg_table_set, dim3(g), dim3(256), 0, s, node_ids, (long)S, (long)N, table, err);
    hipLaunchKernelGGL(k_sg_table_check, dim3(g), dim3(256), 0, s, node_ids, (long)S, (long)N, (const int32_t*)table, err);
  }
  if (hipMemsetAsync(cnt + p.blocks, 0, sizeof(int64_t), s) != hipSuccess) return fail(2, "mgn_subgraph_count: memset");
  if (E > 0)
    hipLaunchKernelGGL(k_sg_flag, dim3((unsigned)p.blocks), dim3(SG_THREADS), 0, s, src, dst, (long)E, (long)N, (const int32_t*)table, ls, ld,
                       cnt, err);
  size_t tb = p.tmp_bytes;
  if (rocprim::exclusive_scan(w + p.tmp, tb, cnt, offs, (int64_t)0, (size_t)p.blocks + 1, rocprim::plus<int64_t>(), s) != hipSuccess)
    return fail(2, "mgn_subgraph_count: scan");
  if (int rc = check_launch("mgn_subgraph_count")) return rc;
  int64_t total = 0;
  int flags = 0;
  if (hipMemcpyAsync(&total, offs + p.blocks, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(2, "mgn_subgraph_count: memcpy");
  if (hipMemcpyAsync(&flags, err, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(2, "mgn_subgraph_count: memcpy");
  if (hipStreamSynchronize(s) != hipSuccess) return fail(2, "mgn_subgraph_count: sync failed");
  if (flags & SG_ERR_RANGE) return fail(3, "mgn_subgraph_count: an entry of node_ids, src or dst is outside [0, N)");
  if (flags & SG_ERR_DUP) return fail(5, "mgn_subgraph_count: node_ids lists a node twice");
  SgHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = SG_MAGIC; h.N = N; h.E = E; h.S = S; h.n_edges = total;
  if (int rc = ws_header_put(w + p.header, &h, sizeof(h), s, "mgn_subgraph_count")) return rc;
  *n_edges_host = total;
  return 0;
}

extern "C" int mgn_subgraph_fill(const void* ws, size_t ws_bytes, int64_t E, int64_t* out_src, int64_t* out_dst, int64_t* out_edge_pos,
                                 uint8_t* out_edge_mask, int64_t cap, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (E < 0 || E > SG_EMAX) return fail(1, "mgn_subgraph_fill: E must be in [0, 2^40]");
  if (cap < 0) return fail(1, "mgn_subgraph_fill: cap must be >= 0");
  if (!ws || ws_bytes < 768) return fail(1, "mgn_subgraph_fill: workspace (ws_bytes) too small");
  const char* w = (const char*)align256((size_t)ws);  // the header fits: 255 + 256 < 768
  SgHeader h;
  if (int rc = ws_header_get(w, &h, sizeof(h), s, "mgn_subgraph_fill")) return rc;
  if (h.magic != SG_MAGIC || h.E != E) return fail(1, "mgn_subgraph_fill: the workspace does not hold a mgn_subgraph_count of this E");
  const SgPlan p = sg_plan(h.N, E);
  if (!ws_base(ws, ws_bytes, p.total)) return fail(1, "mgn_subgraph_fill: workspace (ws_bytes) too small");
  if (cap < h.n_edges) return fail(1, "mgn_subgraph_fill: cap is smaller than the counted number of edges");
  if (h.n_edges > 0 && (!out_src || !out_dst || !out_edge_pos)) return fail(1, "mgn_subgraph_fill: out_src / out_dst / out_edge_pos must not be null");
  if (E == 0) return 0;
  hipLaunchKernelGGL(k_sg_fill, dim3((unsigned)p.blocks), dim3(SG_THREADS), 0, s, (const int32_t*)(w + p.ls), (const int32_t*)(w + p.ld), (long)E,
                     (const int64_t*)(w + p.offs), (long)h.n_edges, out_src, out_dst, out_edge_pos, out_edge_mask);
  return check_launch("mgn_subgraph_fill");
}

extern "C" int mgn_gather_rows_batch(int n_jobs, const mgn_gather_job* jobs, void* stream) {
  if (n_jobs < 0 || n_jobs > MGN_MAX_GATHER_JOBS) return fail(1, "mgn_gather_rows_batch: n_jobs must be in [0, 8]");
  if (n_jobs > 0 && !jobs) return fail(1, "mgn_gather_rows_batch: jobs must not be null");
  SgGatherArgs A;
  memset(&A, 0, sizeof(A));
  int64_t tiles = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const mgn_gather_job& J = jobs[i];
    if (J.rows < 0 || J.src_rows < 0) return fail(1, "mgn_gather_rows_batch: rows / src_rows must be >= 0");
    if (J.width < 1 || J.width > 2147483647LL) return fail(1, "mgn_gather_rows_batch: width must be in [1, 2^31 - 1]");
    if (J.ld_src < J.width || J.ld_dst < J.width) return fail(1, "mgn_gather_rows_batch: ld_src / ld_dst must be >= width");
    if (J.rows == 0) continue;  // nothing to copy: the job takes no workgroup
    if (!J.src || !J.idx || !J.dst) return fail(1, "mgn_gather_rows_batch: src / idx / dst must not be null when rows > 0");
    int64_t tr = SG_GATHER_ELEMS / J.width;
    tr = tr < 1 ? 1 : (tr > SG_GATHER_ROWS ? SG_GATHER_ROWS : tr);
    A.job[A.n] = J;
    A.tile_rows[A.n] = tr;
    A.tile_start[A.n] = tiles;
    tiles += (J.rows + tr - 1) / tr;
    ++A.n;
  }
  A.tile_start[A.n] = tiles;
  if (tiles > 2147483647LL) return fail(1, "mgn_gather_rows_batch: too many rows for one launch");
  if (tiles == 0) return 0;
  hipLaunchKernelGGL(k_sg_gather, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, A);
  return check_launch("mgn_gather_rows_batch");
}
