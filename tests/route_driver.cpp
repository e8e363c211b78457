// Host-only driver of the launch routing in csrc/mgn_kernels.hip: for each case it sets the MGN_* switches, calls the
// public entry point with dummy device addresses (the entry points never dereference them on the host) and prints the
// return code, the error text and every kernel launch in order as `name grid block lds` (a weight-gradient launch also with
// its hand-out of the workgroups).  No HIP runtime is linked and
// no device is opened: the runtime symbols the object needs are defined here.  tests/test_mlp_routes_host.py builds it,
// runs it and compares the output with tests/mlp_routes_expected.txt.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "mgn_kernels.hip"  // (-I csrc)

// the hand-out of a weight-gradient launch: width, interleave and the first workgroup of each job
static std::string wgrad_handout(const WgradLaunch& L) {
  std::string t = " H=" + std::to_string(L.H) + " interleave=" + std::to_string(L.interleave) + " wg0=";
  for (int j = 0; j <= L.njobs; ++j) t += (j ? "," : "") + std::to_string(L.wg0[j]);
  return t;
}

// ---------------------------------------------------------------------------- stand-ins for the HIP runtime
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
// a <<<...>>> launch pushes its configuration, the kernel's host stub pops it and calls hipLaunchKernel
static struct { dim3 grid, block; size_t lds; hipStream_t stream; } g_cfg;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
  g_cfg = {grid, block, lds, stream};
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
  return hipSuccess;
}
// every launch ends here: print it, named through the unit's kernel table, and check its LDS against the reservations so far
static int g_reserved[K_COUNT];
static int g_unreserved = 0;
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
  for (int k = 0; k < K_COUNT; ++k)
    if (kKernels[k].fn == fn && attr == hipFuncAttributeMaxDynamicSharedMemorySize && value > g_reserved[k]) g_reserved[k] = value;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
  const char* name = fn == (const void*)k_colred ? "k_colred" : fn == (const void*)k_colred_batch ? "k_colred_batch" : "?";
  int reserved = 0;
  std::string extra;
  for (int k = 0; k < K_COUNT; ++k)
    if (kKernels[k].fn == fn) {
      name = kKernels[k].name;
      reserved = g_reserved[k];
      if (kKernels[k].sig == SIG_WGRAD) extra = wgrad_handout(*(const WgradLaunch*)args[0]);
    }
  if (grid.y == 1) printf("  %s grid=%u block=%u lds=%zu%s\n", name, grid.x, block.x, lds, extra.c_str());
  else printf("  %s grid=%ux%u block=%u lds=%zu%s\n", name, grid.x, grid.y, block.x, lds, extra.c_str());
  if (lds > 0 && (size_t)reserved < lds) {  // every launch with dynamic LDS follows a reservation of at least that much
    printf("  ^ LDS NOT RESERVED (%d bytes reserved)\n", reserved);
    ++g_unreserved;
  }
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = 0; return hipSuccess; }
}

// ---------------------------------------------------------------------------- cases
static const char* const kSwitches[] = {"MGN_NO_LDS", "MGN_MT", "MGN_GRID", "MGN_FP32_MFMA", "MGN_X6_STATIC", "MGN_PP", "MGN_PPR", "MGN_PPR_XCD",
                                        "MGN_PPR_BWD", "MGN_NW", "MGN_WGRAD_GENERIC_BUDGET", "MGN_WGRAD_NO_ROW64", "MGN_WGRAD_PC",
                                        "MGN_WGRAD_NO_INTERLEAVE", "MGN_WGRAD_ROW64_EXACT"};

// `env` is a blank-separated list of NAME=VALUE without the MGN_ prefix ("PPR=0 PP=2")
static void begin_case(const char* name, const char* env) {
  for (const char* s : kSwitches) unsetenv(s);
  std::string e = env;
  size_t i = 0;
  while (i < e.size()) {
    size_t j = e.find(' ', i);
    if (j == std::string::npos) j = e.size();
    const std::string kv = e.substr(i, j - i);
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) setenv(("MGN_" + kv.substr(0, eq)).c_str(), kv.substr(eq + 1).c_str(), 1);
    i = j + 1;
  }
  printf("== %s%s%s\n", name, *env ? " | " : "", env);
}
static void end_case(int rc) { printf("  rc=%d%s%s\n", rc, rc ? " " : "", rc ? mgn_last_error() : ""); }

// distinct, 16-byte aligned dummy device addresses
template <class T = float>
static T* P(int n) { return (T*)(uintptr_t)(0x100000 + 0x1000 * (uintptr_t)n); }
static const char* const WPK = (const char*)(uintptr_t)0x40000000;

// ---- forward
static mgn_mlp_fwd_args F(int64_t M, int H, int NL) {
  mgn_mlp_fwd_args a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.H = H; a.NL = NL; a.nphase = 1; a.kw[0] = H; a.out_w = H; a.eps = 1e-6f;
  a.src[0] = P(1); a.out = P(2);
  for (int l = 0; l < NL; ++l) { a.W[l] = P(10 + l); a.b[l] = P(20 + l); }
  return a;
}
static mgn_mlp_fwd_args pack(mgn_mlp_fwd_args a) {
  const int G = a.nphase + a.NL - 1 + a.n_post;
  for (int u = 0; u < G && u < 8; ++u) a.wpk[u] = WPK + (size_t)u * MGN_WPACK_BYTES;
  return a;
}
static mgn_mlp_fwd_args saves(mgn_mlp_fwd_args a) {
  a.saveU = P(30); a.saveR = P(31);
  for (int l = 0; l < 3; ++l) { a.saveH[l] = P(32 + l); a.saveM[l] = P<uint32_t>(36 + l); }
  return a;
}
// the edge update of a round: norm, residual, two gathered adds, fused segment sum keyed by the first add's index
static mgn_mlp_fwd_args edge(int64_t M, int precision = 0) {
  mgn_mlp_fwd_args a = F(M, 128, 4);
  a.resid = P(3); a.scale = P(4); a.n_add = 2; a.precision = precision;
  a.add_src[0] = P(40); a.add_src[1] = P(41);
  a.add_idx[0] = P<int32_t>(42); a.add_idx[1] = P<int32_t>(43);
  a.add_rows[0] = a.add_rows[1] = 30000;
  a.seg_out = P(44); a.seg_key = a.add_idx[0]; a.seg_rowptr = P<int32_t>(45); a.seg_part = P(46);
  return pack(a);
}
// the node update: two phases, norm, residual, n_post post-products
static mgn_mlp_fwd_args node(int64_t M, int n_post, int precision = 0) {
  mgn_mlp_fwd_args a = F(M, 128, 4);
  a.nphase = 2; a.kw[1] = 128; a.src[1] = P(5); a.resid = P(3); a.scale = P(4); a.n_post = n_post; a.post_ldw = 128; a.precision = precision;
  for (int q = 0; q < n_post; ++q) { a.post_W[q] = P(50 + q); a.post_out[q] = P(52 + q); }
  return pack(a);
}
static void fwd(const char* name, const char* env, const mgn_mlp_fwd_args& a) {
  begin_case(name, env);
  end_case(mgn_mlp_fwd(&a, nullptr));
}

static void forward_cases() {
  // generic and LDS
  for (int H : {16, 32, 64})
    for (int64_t M : {131071, 131072}) {
      mgn_mlp_fwd_args a = F(M, H, 2);
      fwd(("fwd generic H=" + std::to_string(H) + " M=" + std::to_string(M)).c_str(), "", a);
      a.out_w = 3;
      fwd(("fwd generic H=" + std::to_string(H) + " out_w=3 M=" + std::to_string(M)).c_str(), "", a);
    }
  for (int64_t M : {131071, 131072}) {
    mgn_mlp_fwd_args a = F(M, 128, 4);
    a.kw[0] = 48;
    fwd(("fwd ragged kw=48 M=" + std::to_string(M)).c_str(), "", a);
    a = F(M, 128, 4);
    a.out_w = 16;
    fwd(("fwd ragged out_w=16 M=" + std::to_string(M)).c_str(), "", a);
    a = F(M, 32, 3);
    a.out_w = 3;
    fwd(("fwd ragged H=32 out_w=3 M=" + std::to_string(M)).c_str(), "", a);
  }
  for (int NL : {1, 4, 5}) fwd(("fwd lds NL=" + std::to_string(NL)).c_str(), "", F(180000, 128, NL));
  for (int64_t M : {32768, 32769}) fwd(("fwd lds M=" + std::to_string(M)).c_str(), "", F(M, 128, 4));
  fwd("fwd lds", "MT=2", F(180000, 128, 4));
  fwd("fwd generic H=64 M=1000", "MT=2", F(1000, 64, 2));
  fwd("fwd generic H=64 M=200000", "MT=1", F(200000, 64, 2));
  fwd("fwd lds", "GRID=100", F(180000, 128, 4));
  fwd("fwd lds", "GRID=0", F(180000, 128, 4));
  fwd("fwd lds", "GRID=1000", F(180000, 128, 4));
  fwd("fwd generic H=64", "GRID=100", F(180000, 64, 2));
  fwd("fwd H=128 full", "NO_LDS=1", F(180000, 128, 4));
  fwd("fwd H=128 full M=1000", "NO_LDS=1", F(1000, 128, 4));
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.act = MGN_ACT_GELU; fwd("fwd GELU H=128", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 3); a.act = MGN_ACT_GELU; fwd("fwd GELU H=64", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 3); a.act = MGN_ACT_SILU; fwd("fwd SiLU H=64", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 3); a.precision = 1; fwd("fwd generic H=64 precision 1", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 128, 1); a.kw[0] = 48; a.out_relu = 1; fwd("fwd out_relu ragged", "", a); }
  fwd("fwd M=0", "", F(0, 128, 4));
  // packed, dynamic
  for (int pr : {0, 1, 2}) {
    mgn_mlp_fwd_args a = pack(F(180000, 128, 4));
    a.precision = pr;
    fwd(("fwd packed precision " + std::to_string(pr)).c_str(), "", a);
  }
  for (int pr : {0, 1}) {
    mgn_mlp_fwd_args a = pack(F(180000, 128, 4));
    a.act = MGN_ACT_SILU; a.precision = pr;
    fwd(("fwd packed SiLU precision " + std::to_string(pr)).c_str(), "", a);
    fwd(("fwd packed SiLU precision " + std::to_string(pr)).c_str(), "NW=8", a);
  }
  for (int pr : {0, 1}) {
    mgn_mlp_fwd_args a = pack(F(180000, 128, 4));
    a.precision = pr;
    fwd(("fwd packed precision " + std::to_string(pr)).c_str(), "NW=8", a);
  }
  fwd("fwd packed M=32768", "NW=8", pack(F(32768, 128, 4)));
  fwd("fwd packed M=32769", "NW=8", pack(F(32769, 128, 4)));
  fwd("fwd packed M=32768", "", pack(F(32768, 128, 4)));
  fwd("fwd packed M=32769", "", pack(F(32769, 128, 4)));
  fwd("fwd packed", "NW=8 GRID=100", pack(F(180000, 128, 4)));
  fwd("fwd packed", "GRID=100", pack(F(180000, 128, 4)));
  fwd("fwd packed", "NW=4", pack(F(180000, 128, 4)));
  {
    mgn_mlp_fwd_args a = pack(F(180000, 128, 4));
    a.seg_out = P(44); a.seg_key = P<int32_t>(42); a.seg_rowptr = P<int32_t>(45); a.seg_part = P(46);
    fwd("fwd packed seg_out", "", a);
    fwd("fwd packed seg_out", "NW=8", a);
  }
  fwd("fwd packed", "FP32_MFMA=1", pack(F(180000, 128, 4)));
  fwd("fwd packed", "NO_LDS=1", pack(F(180000, 128, 4)));
  {  // nine units: 3 phases + 4 + 2 post-products
    mgn_mlp_fwd_args a = F(180000, 128, 5);
    a.nphase = 3; a.kw[1] = a.kw[2] = 128; a.src[1] = P(5); a.src[2] = P(6); a.n_post = 2; a.post_ldw = 128;
    a.post_W[0] = P(50); a.post_W[1] = P(51); a.post_out[0] = P(52); a.post_out[1] = P(53);
    fwd("fwd packed nine units", "", pack(a));
    a.n_post = 1;
    fwd("fwd packed eight units", "", pack(a));
  }
  {
    mgn_mlp_fwd_args a = F(180000, 128, 4);
    a.nphase = 2; a.kw[1] = 128; a.src[1] = P(5); a.n_add = 1; a.add_src[0] = P(40);
    fwd("fwd packed n_add=1 two phases", "", pack(a));
    a.nphase = 1;
    fwd("fwd packed n_add=1 one phase", "", pack(a));
    a.NL = 1; a.resid = P(3);
    fwd("fwd packed n_add=1 NL=1 resid", "", pack(a));
  }
  { mgn_mlp_fwd_args a = pack(F(180000, 128, 4)); a.wpk[2] = nullptr; fwd("fwd packed one unit missing", "", a); }
  // packed, static shapes
  for (int pr : {0, 1}) {
    fwd(("fwd edge M=65535 precision " + std::to_string(pr)).c_str(), "", edge(65535, pr));
    fwd(("fwd edge M=65535 precision " + std::to_string(pr)).c_str(), "X6_STATIC=0", edge(65535, pr));
    fwd(("fwd edge M=65535 precision " + std::to_string(pr)).c_str(), "X6_STATIC=2", edge(65535, pr));
  }
  fwd("fwd edge M=65535", "GRID=64", edge(65535));
  { mgn_mlp_fwd_args a = edge(65535); a.seg_key = P<int32_t>(47); fwd("fwd edge seg_key != add_idx[0]", "", a); }
  { mgn_mlp_fwd_args a = edge(65535); a.idx[0] = P<int32_t>(48); fwd("fwd edge idx[0] set", "", a); }
  { mgn_mlp_fwd_args a = edge(65535); a.scale = nullptr; fwd("fwd edge no norm", "", a); }
  for (int n_post : {2, 0})
    for (int64_t M : {131071, 131072})
      for (int pr : {0, 1}) {
        const std::string n = "fwd node n_post=" + std::to_string(n_post) + " M=" + std::to_string(M) + " precision " + std::to_string(pr);
        fwd(n.c_str(), "", node(M, n_post, pr));
      }
  fwd("fwd node n_post=2 M=131072", "X6_STATIC=0", node(131072, 2));
  fwd("fwd node n_post=2 M=131072", "X6_STATIC=2", node(131072, 2));
  fwd("fwd node n_post=0 M=131072", "X6_STATIC=2", node(131072, 0));
  fwd("fwd node n_post=1 M=131072", "", node(131072, 1));
  fwd("fwd node n_post=2 M=131072", "NW=8", node(131072, 2));
  for (int64_t M : {96, 97, 512 * 96, 512 * 96 + 1}) fwd(("fwd edge M=" + std::to_string(M)).c_str(), "NW=6", edge(M));
  fwd("fwd edge M=65535 precision 1", "NW=6", edge(65535, 1));
  fwd("fwd edge M=65536", "NW=6", edge(65536));
  fwd("fwd edge M=65536", "NW=6 PPR=0 PP=1", edge(65536));
  fwd("fwd node n_post=2 M=131072", "NW=6", node(131072, 2));
  fwd("fwd packed", "NW=6", pack(F(180000, 128, 4)));
  // ppr and pp on the edge shape
  for (int64_t M : {65535, 65536}) {
    fwd(("fwd edge M=" + std::to_string(M)).c_str(), "", edge(M));
    fwd(("fwd edge saves M=" + std::to_string(M)).c_str(), "", saves(edge(M)));
  }
  fwd("fwd edge M=180000", "", edge(180000));
  fwd("fwd edge M=65536", "PPR=0", edge(65536));
  fwd("fwd edge M=1", "PPR=2", edge(1));
  fwd("fwd edge M=33", "PPR=2", edge(33));
  fwd("fwd edge M=8161", "PPR=2", edge(8161));
  fwd("fwd edge M=8193", "PPR=2", edge(8193));
  fwd("fwd edge M=65536", "PPR_XCD=0", edge(65536));
  fwd("fwd edge saves M=65536", "PPR_XCD=0", saves(edge(65536)));
  fwd("fwd edge M=65536", "PPR_XCD=1", edge(65536));
  { mgn_mlp_fwd_args a = saves(edge(65536)); a.saveM[1] = nullptr; fwd("fwd edge one save missing M=65536", "", a); }
  { mgn_mlp_fwd_args a = edge(65536); a.out = (float*)a.resid; fwd("fwd edge out == resid", "", a); }
  { mgn_mlp_fwd_args a = edge(65536); a.out = (float*)a.src[0]; fwd("fwd edge out == src[0]", "", a); }
  { mgn_mlp_fwd_args a = edge(65536); a.y_out = P(7); fwd("fwd edge y_out", "", a); }
  fwd("fwd edge precision 1 M=65536", "", edge(65536, 1));
  fwd("fwd edge M=2^23-1", "", edge(((int64_t)1 << 23) - 1));
  fwd("fwd edge M=2^23", "", edge((int64_t)1 << 23));
  fwd("fwd edge M=2^23", "PPR=0 PP=1", edge((int64_t)1 << 23));
  for (int q : {0, 1}) {
    mgn_mlp_fwd_args a = edge(65536);
    a.add_rows[q] = 0;
    fwd(("fwd edge add_rows[" + std::to_string(q) + "]=0").c_str(), "", a);
    a.add_rows[q] = (int64_t)1 << 23;
    fwd(("fwd edge add_rows[" + std::to_string(q) + "]=2^23").c_str(), "", a);
    a.add_rows[q] = ((int64_t)1 << 23) - 1;
    fwd(("fwd edge add_rows[" + std::to_string(q) + "]=2^23-1").c_str(), "", a);
  }
  { mgn_mlp_fwd_args a = edge(65536); a.wpk[2] = WPK + 5 * (size_t)MGN_WPACK_BYTES; fwd("fwd edge units not back to back", "", a); fwd("fwd edge units not back to back", "PPR=0 PP=1", a); }
  fwd("fwd edge inference M=65536", "PPR=0", edge(65536));
  fwd("fwd edge inference M=65535", "PPR=0", edge(65535));
  fwd("fwd edge training M=65536", "PPR=0", saves(edge(65536)));
  fwd("fwd edge inference M=65536", "PPR=0 PP=0", edge(65536));
  fwd("fwd edge inference M=65536", "PPR=0 PP=1", edge(65536));
  fwd("fwd edge training M=65536", "PPR=0 PP=1", saves(edge(65536)));
  fwd("fwd edge training M=65535", "PPR=0 PP=1", saves(edge(65535)));
  fwd("fwd edge inference M=1", "PPR=0 PP=2", edge(1));
  fwd("fwd edge training M=1", "PPR=0 PP=2", saves(edge(1)));
  fwd("fwd edge inference M=32769", "PPR=0 PP=2", edge(32769));
  { mgn_mlp_fwd_args a = saves(edge(65536)); a.saveH[2] = nullptr; fwd("fwd edge one save missing M=65536", "PPR=0 PP=1", a); }
  { mgn_mlp_fwd_args a = edge(65536); a.out = (float*)a.resid; fwd("fwd edge out == resid", "PPR=0 PP=1", a); }
  { mgn_mlp_fwd_args a = edge(65536); a.y_out = P(7); fwd("fwd edge y_out", "PPR=0 PP=1", a); }
  fwd("fwd edge precision 1 M=65536", "PPR=0 PP=1", edge(65536, 1));
  // refusals, in the order of the entry point
  { mgn_mlp_fwd_args a = F(1000, 48, 2); fwd("fwd refusal H", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.NL = 0; fwd("fwd refusal NL", "", a); a.NL = 9; fwd("fwd refusal NL=9", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.out_w = 65; fwd("fwd refusal out_w", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.precision = 3; fwd("fwd refusal precision", "", a); }
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.precision = 2; fwd("fwd refusal precision 2 not packed", "", a); }
  { mgn_mlp_fwd_args a = pack(F(180000, 128, 4)); a.precision = 2; fwd("fwd refusal precision 2", "FP32_MFMA=1", a); fwd("fwd refusal precision 2", "NO_LDS=1", a);
    a.act = MGN_ACT_SILU; fwd("fwd refusal precision 2 SiLU", "", a); }
  { mgn_mlp_fwd_args a = pack(F(180000, 64, 4)); a.precision = 2; fwd("fwd refusal precision 2 H=64", "", a); }
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.seg_out = P(44); a.seg_key = P<int32_t>(42); a.seg_rowptr = P<int32_t>(45); a.seg_part = P(46);
    fwd("fwd refusal seg_out not packed", "", a);
    a = pack(a); a.seg_part = nullptr; fwd("fwd refusal seg_out without seg_part", "", a);
    a.seg_part = P(46); a.act = MGN_ACT_GELU; fwd("fwd refusal seg_out GELU (plan without act)", "", a); }
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.out_relu = 1; fwd("fwd refusal out_relu on lds", "", a); a.act = MGN_ACT_GELU; fwd("fwd refusal out_relu GELU H=128 (plan without act)", "", a);
    a = F(1000, 64, 2); a.out_relu = 1; a.resid = P(3); fwd("fwd refusal out_relu resid", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.act = 3; fwd("fwd refusal act", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.act = MGN_ACT_GELU; a.precision = 1; fwd("fwd refusal GELU precision 1", "", a); }
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.act = MGN_ACT_SILU; fwd("fwd refusal SiLU lds", "", a); fwd("fwd SiLU H=128 generic", "NO_LDS=1", a);
    a.NL = 1; fwd("fwd SiLU lds NL=1", "", a); }
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.precision = 1; fwd("fwd refusal precision 1 lds", "", a); fwd("fwd precision 1 H=128 generic", "NO_LDS=1", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.nphase = 0; fwd("fwd refusal nphase", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.kw[0] = 0; fwd("fwd refusal kw", "", a); a.kw[0] = 65; fwd("fwd refusal kw=65", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.scale = P(4); a.out_w = 48; fwd("fwd refusal norm out_w", "", a); }
  { mgn_mlp_fwd_args a = F(180000, 128, 4); a.n_add = 3; fwd("fwd refusal n_add", "", a); a.n_add = 0; a.n_post = -1; fwd("fwd refusal n_post", "", a); }
  { mgn_mlp_fwd_args a = F(1000, 64, 2); a.n_add = 1; fwd("fwd refusal n_add H=64", "", a);
    a = F(180000, 128, 4); a.ldw0 = 384; fwd("fwd refusal ldw0", "NO_LDS=1", a); fwd("fwd ldw0 lds", "", a);
    a.act = MGN_ACT_GELU; a.ldw0 = 0; a.n_post = 0; fwd("fwd GELU H=128 passes the extension check (plan without act)", "", a); }
}

// ---- backward
static mgn_mlp_bwd_args B(int64_t M, int H, int NL) {
  mgn_mlp_bwd_args a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.H = H; a.NL = NL; a.out_w = H; a.eps = 1e-6f; a.dOut = P(1); a.n_din = 1;
  a.WT0[0] = P(2); a.dIn[0] = P(3);
  for (int l = 0; l < NL; ++l) { a.WT[l] = P(10 + l); a.dZ[l] = P(20 + l); a.db[l] = P(30 + l); }
  for (int l = 1; l < NL; ++l) a.Hs[l - 1] = P(40 + l);
  a.red_ws = P(60); a.red_ws_bytes = (size_t)1 << 40;
  return a;
}
static mgn_mlp_bwd_args pack(mgn_mlp_bwd_args a) {
  const int G = a.n_front + a.NL - 1 + a.n_din;
  for (int u = 0; u < G && u < 8; ++u) a.wpk[u] = WPK + (size_t)u * MGN_WPACK_BYTES;
  for (int l = 1; l < a.NL; ++l) { a.Ms[l - 1] = P<uint32_t>(70 + l); a.Zs[l - 1] = nullptr; }
  return a;
}
// the edge chain of a round: norm, input residual, gathered second gradient, only dscale as a column sum
static mgn_mlp_bwd_args edge_chain(int64_t M, int precision = 0) {
  mgn_mlp_bwd_args a = B(M, 128, 4);
  a.scale = P(4); a.dscale = P(5); a.U = P(6); a.R = P(7); a.din_resid[0] = P(8); a.dOut2 = P(9); a.idx2 = P<int32_t>(50); a.dOut2_rows = 30000;
  a.precision = precision;
  for (int l = 0; l < 4; ++l) a.db[l] = nullptr;
  return pack(a);
}
static void bwd(const char* name, const char* env, const mgn_mlp_bwd_args& a) {
  begin_case(name, env);
  end_case(mgn_mlp_bwd(&a, nullptr));
}

static void backward_cases() {
  for (int H : {16, 32, 64})
    for (int64_t M : {131071, 131072}) {
      mgn_mlp_bwd_args a = B(M, H, 2);
      bwd(("bwd generic H=" + std::to_string(H) + " M=" + std::to_string(M)).c_str(), "", a);
      a.out_w = 3;
      bwd(("bwd generic H=" + std::to_string(H) + " out_w=3 M=" + std::to_string(M)).c_str(), "", a);
    }
  for (int64_t M : {131071, 131072}) {
    mgn_mlp_bwd_args a = B(M, 128, 4);
    a.out_w = 16;
    bwd(("bwd out_w=16 H=128 M=" + std::to_string(M)).c_str(), "", a);
    a = B(M, 64, 3);
    a.out_w = 3;
    bwd(("bwd out_w=3 H=64 M=" + std::to_string(M)).c_str(), "", a);
    a = B(M, 128, 4);
    a.n_din = 2; a.WT0[1] = P(52); a.dIn[1] = P(53);
    bwd(("bwd n_din=2 H=128 M=" + std::to_string(M)).c_str(), "", a);
    bwd(("bwd lds M=" + std::to_string(M)).c_str(), "", B(M, 128, 4));
  }
  bwd("bwd lds M=32768", "", B(32768, 128, 4));
  bwd("bwd lds M=32769", "", B(32769, 128, 4));
  bwd("bwd H=128 NL=1", "", B(180000, 128, 1));
  bwd("bwd lds NL=2", "", B(180000, 128, 2));
  bwd("bwd H=128 NL=5", "", B(180000, 128, 5));
  bwd("bwd lds", "MT=2", B(180000, 128, 4));
  bwd("bwd lds", "GRID=100", B(180000, 128, 4));
  bwd("bwd H=128 full", "NO_LDS=1", B(180000, 128, 4));
  bwd("bwd generic H=64 M=1000", "MT=2", B(1000, 64, 2));
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.act = MGN_ACT_GELU; for (int l = 1; l < 4; ++l) a.Zs[l - 1] = P(80 + l); bwd("bwd GELU H=128", "", a);
    a.defer_reduce = 1; bwd("bwd GELU H=128 deferred", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 3); a.act = MGN_ACT_SILU; for (int l = 1; l < 3; ++l) a.Zs[l - 1] = P(80 + l); bwd("bwd SiLU H=64", "", a); }
  bwd("bwd M=0", "", B(0, 128, 4));
  // packed
  for (int pr : {0, 1, 2, 3}) {
    mgn_mlp_bwd_args a = pack(B(180000, 128, 4));
    a.precision = pr;
    bwd(("bwd packed precision " + std::to_string(pr)).c_str(), "", a);
  }
  bwd("bwd packed", "FP32_MFMA=1", pack(B(180000, 128, 4)));
  bwd("bwd packed", "NO_LDS=1", pack(B(180000, 128, 4)));
  bwd("bwd packed", "GRID=100", pack(B(180000, 128, 4)));
  bwd("bwd packed M=32769", "", pack(B(32769, 128, 4)));
  bwd("bwd packed M=1000", "", pack(B(1000, 128, 4)));
  for (int pr : {0, 1}) {
    mgn_mlp_bwd_args a = B(180000, 128, 4);
    a.n_front = 2; a.front_src[0] = P(54); a.front_src[1] = P(55); a.front_out = P(56); a.precision = pr;
    bwd(("bwd packed front stage precision " + std::to_string(pr)).c_str(), "", pack(a));
  }
  for (int pr : {0, 1}) {
    mgn_mlp_bwd_args a = pack(B(180000, 128, 4));
    a.act = MGN_ACT_SILU; a.precision = pr;
    for (int l = 1; l < 4; ++l) { a.Zs[l - 1] = P(80 + l); a.Ms[l - 1] = nullptr; }
    bwd(("bwd packed SiLU precision " + std::to_string(pr)).c_str(), "", a);
  }
  {
    mgn_mlp_bwd_args a = pack(B(180000, 128, 4));
    a.seg_out = P(44); a.seg_key = P<int32_t>(42); a.seg_rowptr = P<int32_t>(45); a.seg_part = P(46);
    bwd("bwd packed fused segment sum", "", a);
  }
  {  // column-sum slots: 0, 1 and 5
    mgn_mlp_bwd_args a = pack(B(180000, 128, 4));
    for (int l = 0; l < 4; ++l) a.db[l] = nullptr;
    bwd("bwd packed no column sums", "", a);
    a.scale = P(4); a.dscale = P(5); a.U = P(6); a.R = P(7);
    bwd("bwd packed dscale only", "", a);
    for (int l = 0; l < 4; ++l) a.db[l] = P(30 + l);
    bwd("bwd packed five column sums", "", a);
    a.defer_reduce = 1;
    bwd("bwd packed five column sums deferred", "", a);
    a.defer_reduce = 0; a.scale = nullptr;
    bwd("bwd packed dscale without scale", "", a);
  }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.defer_reduce = 1; bwd("bwd lds deferred", "", a);
    for (int l = 0; l < 4; ++l) a.db[l] = nullptr; a.defer_reduce = 0; bwd("bwd lds no reduction output", "", a); }
  { mgn_mlp_bwd_args a = pack(B(180000, 128, 4)); a.Ms[1] = nullptr; bwd("bwd packed Ms missing", "", a); }
  { mgn_mlp_bwd_args a = pack(B(180000, 128, 4)); a.wpk[1] = nullptr; bwd("bwd packed one unit missing", "", a); }
  // the edge chain
  for (int pr : {0, 1}) {
    bwd(("bwd edge chain M=65535 precision " + std::to_string(pr)).c_str(), "", edge_chain(65535, pr));
    bwd(("bwd edge chain M=65536 precision " + std::to_string(pr)).c_str(), "", edge_chain(65536, pr));
    bwd(("bwd edge chain M=65536 precision " + std::to_string(pr)).c_str(), "X6_STATIC=0", edge_chain(65536, pr));
    bwd(("bwd edge chain M=65536 precision " + std::to_string(pr)).c_str(), "PPR_BWD=0", edge_chain(65536, pr));
  }
  bwd("bwd edge chain M=65536", "X6_STATIC=2", edge_chain(65536));
  bwd("bwd edge chain M=65536", "PPR=0", edge_chain(65536));
  bwd("bwd edge chain M=65536", "PPR_BWD=1", edge_chain(65536));
  bwd("bwd edge chain M=65536", "PPR_XCD=0", edge_chain(65536));
  bwd("bwd edge chain M=65536", "PPR_XCD=0 PPR_BWD=0", edge_chain(65536));
  bwd("bwd edge chain M=180000", "", edge_chain(180000));
  bwd("bwd edge chain M=2^23-1", "", edge_chain(((int64_t)1 << 23) - 1));
  bwd("bwd edge chain M=2^23", "", edge_chain((int64_t)1 << 23));
  { mgn_mlp_bwd_args a = edge_chain(65536); a.db[2] = P(32); bwd("bwd edge chain db[2] set", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.dZ[1] = nullptr; bwd("bwd edge chain dZ[1] missing", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.dscale = nullptr; bwd("bwd edge chain no dscale", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.dOut2_rows = 0; bwd("bwd edge chain dOut2_rows=0", "", a);
    a.dOut2_rows = (int64_t)1 << 23; bwd("bwd edge chain dOut2_rows=2^23", "", a);
    a.dOut2_rows = ((int64_t)1 << 23) - 1; bwd("bwd edge chain dOut2_rows=2^23-1", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.dIn[0] = (float*)a.din_resid[0]; bwd("bwd edge chain dIn[0] == din_resid[0]", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.dZ[3] = (float*)a.dOut; bwd("bwd edge chain dZ[3] == dOut", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.wpk[3] = WPK + 7 * (size_t)MGN_WPACK_BYTES; bwd("bwd edge chain units not back to back", "", a); }
  { mgn_mlp_bwd_args a = edge_chain(65536); a.idx2 = nullptr; bwd("bwd edge chain no idx2", "", a); }
  bwd("bwd edge chain M=33", "PPR=2", edge_chain(33));
  bwd("bwd edge chain M=1", "PPR=2", edge_chain(1));
  bwd("bwd edge chain M=8193", "PPR=2", edge_chain(8193));
  bwd("bwd edge chain M=20000", "PPR=2", edge_chain(20000));
  // refusals, in the order of the entry point
  bwd("bwd refusal H", "", B(1000, 48, 2));
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.NL = 0; bwd("bwd refusal NL", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.out_w = 0; bwd("bwd refusal out_w", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.n_din = 4; bwd("bwd refusal n_din", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.n_din = 2; a.dZ[0] = nullptr; bwd("bwd refusal n_din=2 without dZ[0]", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.precision = 4; bwd("bwd refusal precision", "", a); }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.precision = 2; bwd("bwd refusal precision 2 not packed", "", a);
    a = pack(a); bwd("bwd refusal precision 2", "NO_LDS=1", a); bwd("bwd refusal precision 2", "FP32_MFMA=1", a);
    a.n_front = 1; a.front_src[0] = P(54); bwd("bwd refusal precision 2 front stage", "", pack(a)); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.act = -1; bwd("bwd refusal act", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.act = MGN_ACT_GELU; a.precision = 1; bwd("bwd refusal GELU precision 1", "", a); }
  { mgn_mlp_bwd_args a = B(1000, 64, 2); a.act = MGN_ACT_SILU; bwd("bwd refusal SiLU without Zs", "", a); }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.act = MGN_ACT_SILU; for (int l = 1; l < 4; ++l) a.Zs[l - 1] = P(80 + l); bwd("bwd refusal SiLU lds", "", a);
    bwd("bwd SiLU H=128 generic", "NO_LDS=1", a); }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.n_front = 1; a.front_src[0] = P(54); bwd("bwd refusal front stage not packed", "", a);
    a = pack(a); bwd("bwd refusal front stage", "NO_LDS=1", a); a.dOut2 = P(9); bwd("bwd refusal front stage with dOut2", "", a); }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.precision = 1; bwd("bwd refusal precision 1 lds", "", a); bwd("bwd precision 1 H=128 generic", "NO_LDS=1", a); }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.seg_out = P(44); a.seg_key = P<int32_t>(42); a.seg_rowptr = P<int32_t>(45); a.seg_part = P(46);
    bwd("bwd refusal seg_out not packed", "", a);
    a = pack(a); a.precision = 1; bwd("bwd refusal seg_out precision 1", "", a); }
  { mgn_mlp_bwd_args a = B(180000, 128, 4); a.red_ws_bytes = 1024; bwd("bwd refusal workspace", "", a); }
}

static void colred_cases() {
  mgn_colred_job j[40];
  memset(j, 0, sizeof(j));
  for (int i = 0; i < 40; ++i) {
    j[i].red_ws = P(60 + i); j[i].M = (i & 1) ? 30000 : 180000; j[i].H = 128; j[i].NL = 4; j[i].out_w = 128; j[i].n_din = 1;
    j[i].db[0] = P(30); j[i].dscale = P(5);
  }
  begin_case("colred two jobs", "");
  end_case(mgn_colred_batch(2, j, nullptr));
  begin_case("colred two jobs", "NO_LDS=1");
  end_case(mgn_colred_batch(2, j, nullptr));
  begin_case("colred two jobs", "MT=2");
  end_case(mgn_colred_batch(2, j, nullptr));
  begin_case("colred 40 jobs", "");
  end_case(mgn_colred_batch(40, j, nullptr));
  j[1].H = 64; j[1].NL = 2; j[1].M = 200000;
  begin_case("colred H=128 and H=64", "");
  end_case(mgn_colred_batch(2, j, nullptr));
  begin_case("colred no jobs", "");
  end_case(mgn_colred_batch(0, j, nullptr));
  begin_case("colred refusal n", "");
  end_case(mgn_colred_batch(-1, j, nullptr));
  j[1].NL = 9;
  begin_case("colred refusal job", "");
  end_case(mgn_colred_batch(2, j, nullptr));
  j[0].red_ws = nullptr;
  begin_case("colred refusal job without red_ws", "");
  end_case(mgn_colred_batch(1, j, nullptr));
}

// ---- weight gradients
static mgn_wgrad_job J(int64_t M, int nja, int nkb, int kw, int lda, int ldb, int n = 0) {
  mgn_wgrad_job j;
  memset(&j, 0, sizeof(j));
  j.A = P(100 + 3 * n); j.B = P(101 + 3 * n); j.dW = P(102 + 3 * n); j.M = M; j.lda = lda; j.ldb = ldb; j.ldw = 16 * nkb; j.nja = nja; j.nkb = nkb; j.kw = kw;
  return j;
}
static mgn_wgrad_job full(int64_t M, int n = 0) { return J(M, 8, 8, 128, 128, 128, n); }
static void wg(const char* name, const char* env, const std::vector<mgn_wgrad_job>& jobs, int precision = 0, size_t ws_bytes = (size_t)1 << 40) {
  begin_case(name, env);
  printf("  workspace_bytes=%zu\n", mgn_wgrad_workspace_bytes((int)jobs.size(), jobs.data()));
  end_case(mgn_wgrad_p((int)jobs.size(), jobs.data(), P(90), ws_bytes, precision, nullptr));
}

static void wgrad_cases() {
  wg("wgrad one full job", "", {full(180000)});
  wg("wgrad one full job", "WGRAD_PC=0", {full(180000)});
  wg("wgrad one full job", "WGRAD_PC=1", {full(180000)});
  wg("wgrad one full job", "FP32_MFMA=1", {full(180000)});
  wg("wgrad one full job", "NO_LDS=1", {full(180000)});
  wg("wgrad one full job precision 1", "", {full(180000)}, 1);
  wg("wgrad one full job precision 1", "FP32_MFMA=1", {full(180000)}, 1);
  { mgn_wgrad_job j = full(180000); j.ldb = -128; wg("wgrad full job ldb=-128 precision 1", "", {j}, 1); }
  { mgn_wgrad_job j = full(180000); j.lda = -128; wg("wgrad full job lda=-128 precision 0 (pc off)", "FP32_MFMA=1", {j}, 0); }
  wg("wgrad full job M=8192 (share 64)", "", {full(8192)});
  wg("wgrad full job M=8193 (share 65)", "", {full(8193)});
  wg("wgrad full job M=16384 (share 128)", "WGRAD_PC=0", {full(16384)});
  wg("wgrad full job M=8192 (share 64)", "WGRAD_PC=0", {full(8192)});
  {  // a round of the default block: 16 full jobs over edge and node rows, 6 small ones of the encoders / decoder
    std::vector<mgn_wgrad_job> r;
    for (int i = 0; i < 10; ++i) r.push_back(full(180000, i));
    for (int i = 10; i < 16; ++i) r.push_back(full(30000, i));
    r.push_back(J(180000, 8, 1, 3, 128, 16, 16));
    r.push_back(J(30000, 8, 1, 9, 128, 16, 17));
    r.push_back(J(30000, 1, 8, 128, 16, 128, 18));
    for (int i = 19; i < 22; ++i) r.push_back(J(30000, 8, 4, 64, 128, 64, i));
    wg("wgrad 22-job round", "", r);
    wg("wgrad 22-job round precision 1", "", r, 1);
    wg("wgrad 22-job round", "WGRAD_PC=0", r);
    wg("wgrad 22-job round", "NO_LDS=1", r);
    wg("wgrad 22-job round", "WGRAD_GENERIC_BUDGET=1024", r);
  }
  // small jobs on the generic kernel
  wg("wgrad generic HB=1 (kw=15)", "", {J(30000, 1, 1, 15, 16, 16)});
  wg("wgrad generic HB=2 (kw=30)", "", {J(30000, 2, 2, 30, 32, 32)});
  wg("wgrad generic HB=4 (kw=62)", "", {J(30000, 4, 4, 62, 64, 64)});
  wg("wgrad generic HB=8", "", {J(30000, 8, 4, 64, 128, 64)});
  { mgn_wgrad_job j = J(30000, 4, 4, 64, 64, 64); j.A = (const float*)((const char*)j.A + 4); wg("wgrad generic HB=4 (misaligned A)", "", {j}); }
  { mgn_wgrad_job j = J(30000, 2, 2, 32, 33, 32); wg("wgrad generic HB=2 (lda=33)", "", {j}); }
  // the row-vector kernel
  wg("wgrad row64 full (nja=4, kw=64)", "", {J(30000, 4, 4, 64, 64, 64)});
  wg("wgrad row64 not full (nja=2)", "", {J(30000, 4, 4, 64, 64, 64), J(20000, 2, 4, 64, 32, 64, 1)});
  wg("wgrad row64 not full (kw=60)", "", {J(30000, 4, 4, 60, 64, 64)});
  wg("wgrad row64 full", "WGRAD_ROW64_EXACT=1", {J(30000, 4, 4, 64, 64, 64)});
  wg("wgrad row64 full", "FP32_MFMA=1", {J(30000, 4, 4, 64, 64, 64)});
  wg("wgrad row64 full", "WGRAD_NO_ROW64=1", {J(30000, 4, 4, 64, 64, 64)});
  wg("wgrad row64 HB=1 job", "", {J(30000, 1, 1, 16, 16, 16)});
  wg("wgrad row64 precision 1 neither", "", {J(30000, 4, 4, 64, 64, 64)}, 1);
  wg("wgrad row64 precision 1 A", "", {J(30000, 4, 4, 64, -64, 64)}, 1);
  wg("wgrad row64 precision 1 B", "", {J(30000, 4, 4, 64, 64, -64)}, 1);
  wg("wgrad row64 precision 1 both", "", {J(30000, 4, 4, 64, -64, -64)}, 1);
  wg("wgrad row64 precision 1", "WGRAD_ROW64_EXACT=1", {J(30000, 4, 4, 64, 64, 64)}, 1);
  // interleave
  {
    std::vector<mgn_wgrad_job> r;
    for (int i = 0; i < 4; ++i) r.push_back(J(30000, 4, 4, 64, 64, 64, i));
    wg("wgrad row64 four equal jobs", "", r);
    wg("wgrad row64 four equal jobs", "WGRAD_NO_INTERLEAVE=1", r);
    wg("wgrad row64 four equal jobs", "WGRAD_GENERIC_BUDGET=64", r);
    r[2].M = 29999;
    wg("wgrad row64 four jobs, unequal M", "", r);
    for (auto& j : r) j.M = 8192;
    wg("wgrad row64 four equal jobs M=8192", "", r);
    for (auto& j : r) j.M = 2000;
    wg("wgrad row64 four equal jobs M=2000 (fewer workgroups per job)", "", r);
    for (auto& j : r) j.M = 496;
    wg("wgrad row64 four equal jobs M=496 (too few tiles)", "", r);
    for (auto& j : r) j.M = 512;
    wg("wgrad row64 four equal jobs M=512", "", r);
    r.clear();
    for (int i = 0; i < 9; ++i) r.push_back(J(30000, 4, 4, 64, 64, 64, i));
    wg("wgrad row64 nine equal jobs", "", r);
    r.resize(8);
    wg("wgrad row64 eight equal jobs", "", r);
    r.resize(2);
    wg("wgrad row64 two equal jobs", "", r);
  }
  // the generic budget
  {
    std::vector<mgn_wgrad_job> r = {J(100000, 2, 2, 30, 32, 32), J(50000, 2, 2, 30, 32, 32, 1)};
    wg("wgrad generic two jobs", "", r);
    wg("wgrad generic two jobs", "WGRAD_GENERIC_BUDGET=63", r);
    wg("wgrad generic two jobs", "WGRAD_GENERIC_BUDGET=64", r);
    wg("wgrad generic two jobs", "WGRAD_GENERIC_BUDGET=1024", r);
    wg("wgrad generic two jobs", "WGRAD_GENERIC_BUDGET=1025", r);
    wg("wgrad two full jobs", "WGRAD_GENERIC_BUDGET=64", {full(100000), full(50000, 1)});
  }
  wg("wgrad generic one job M=1040 (share 65)", "", {J(1040 * 4, 2, 2, 30, 32, 32)});
  wg("wgrad generic one job M=4096 (share 64)", "", {J(4096, 2, 2, 30, 32, 32)});
  wg("wgrad generic one job M=4097 (share 65)", "", {J(4097, 2, 2, 30, 32, 32)});
  wg("wgrad job with M=0", "", {J(0, 2, 2, 30, 32, 32)});
  // refusals, in the order of the entry point
  wg("wgrad refusal precision", "", {full(1000)}, 2);
  wg("wgrad refusal njobs", "", {});
  wg("wgrad refusal njobs=49", "", std::vector<mgn_wgrad_job>(49, full(1000)));
  { mgn_wgrad_job j = full(180000); j.ldb = -128; wg("wgrad refusal ldb=-128 precision 0", "", {j}, 0); wg("wgrad refusal ldb=-128", "FP32_MFMA=1", {j}, 1);
    wg("wgrad refusal ldb=-128", "NO_LDS=1", {j}, 1); }
  wg("wgrad refusal bf16 rows, row64 off", "WGRAD_NO_ROW64=1", {J(30000, 4, 4, 64, -64, 64)}, 1);
  wg("wgrad refusal bf16 rows, HB=8 job", "", {J(30000, 8, 4, 64, -128, 64)}, 1);
  wg("wgrad refusal block counts", "", {J(30000, 0, 4, 64, 64, 64)});
  wg("wgrad refusal block counts nkb=9", "", {full(1000), J(30000, 4, 9, 64, 64, 64, 1)});
  wg("wgrad refusal bf16 rows beside a generic job", "", {J(30000, 4, 4, 64, -64, 64), J(30000, 4, 4, 62, 64, 64, 1)}, 1);
  wg("wgrad refusal workspace", "", {full(180000)}, 0, 1024);
  wg("wgrad refusal workspace of the second pass", "", {full(180000), J(30000, 4, 4, 64, 64, 64, 1)}, 0, (size_t)256 * (128 * 128 + 128) * 4);
  wg("wgrad refusal operands disagree", "", {J(30000, 4, 4, 64, -64, 64), J(30000, 4, 4, 64, 64, 64, 1)}, 1);
}

int main() {
  forward_cases();
  backward_cases();
  colred_cases();
  wgrad_cases();
  return g_unreserved ? 1 : 0;
}
