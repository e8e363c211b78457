// Host-only scaffolding of libmgn_hip.so, included by every translation unit: the error channel, the 256-byte workspace
// carving and the header that carries a count call's result to the fill call that follows.  Everything is `static`, so each
// unit has its own thread_local message buffer behind its own mgn_*_last_error: calls that failed in different units do not
// overwrite each other's message.  No device code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

// ---------------------------------------------------------------------------------------- error channel
static thread_local char g_err[256] = "";
static inline int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
static inline int failf(int code, const char* who, const char* what) {  // "<who>: <what>"
  snprintf(g_err, sizeof(g_err), "%s: %s", who, what);
  return code;
}
static inline int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? failf(2, what, hipGetErrorString(e)) : 0;
}

// ---------------------------------------------------------------------------------------- workspace carving
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// bump allocator over offsets: every block starts on a multiple of 256 bytes, `end` is the first byte behind the last block
struct WsCarver {
  size_t end = 0;
  size_t take(size_t bytes) {
    const size_t at = align256(end);
    end = at + bytes;
    return at;
  }
};

// the 256-byte aligned base inside a caller's workspace, or null when ws is null or `need` bytes do not fit behind the base
// (the *_workspace_bytes queries add 256 to their plan's total for this shift)
static inline char* ws_base(const void* ws, size_t ws_bytes, size_t need) {
  const size_t base = align256((size_t)ws);
  return (ws && ws_bytes >= (base - (size_t)ws) + need) ? (char*)base : nullptr;
}

// ---------------------------------------------------------------------------------------- count -> fill header
// The first 256 bytes at the base of a workspace hold a small struct whose first member is a magic number: what a *_fill call
// needs from the *_count call before it.  count clears it first (a failed count leaves no stale header; `bytes` may take in
// flag words that lie directly behind it) and writes it last; fill reads it back.  Both copies use a struct on the caller's
// stack, hence the synchronise.  `who` prefixes the message of a failure.
static inline int ws_header_clear(char* w, size_t bytes, hipStream_t s, const char* who) {
  return hipMemsetAsync(w, 0, bytes, s) != hipSuccess ? failf(2, who, "memset") : 0;
}
static inline int ws_header_put(char* w, const void* h, size_t bytes, hipStream_t s, const char* who) {
  if (hipMemcpyAsync(w, h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return failf(2, who, "memcpy");
  return hipStreamSynchronize(s) != hipSuccess ? failf(2, who, "sync failed") : 0;
}
static inline int ws_header_get(const char* w, void* h, size_t bytes, hipStream_t s, const char* who) {
  if (hipMemcpyAsync(h, w, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return failf(2, who, "memcpy");
  return hipStreamSynchronize(s) != hipSuccess ? failf(2, who, "sync failed") : 0;
}
