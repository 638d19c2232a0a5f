// abc_buffers.hip -- the driver side of the buffer table (abc_buffers.hpp): the caching allocator behind abc_hip_malloc /
// abc_hip_free, the lifetime of recorded circuits (abc_hip_graph_*), the scratch arenas and the mirrors of key-switching keys.
// Every device buffer a recorded circuit may have baked into its kernel arguments is entered here and leaves here; the table
// decides who owns what, this file calls hipMalloc / hipFree.  Table calls are made under alloc_mu.  Under ABC_HIP_POISON=1 (debug)
// it also fills what it hands out -- caller blocks and scratch arenas, never keys or their mirrors -- with 0xFF bytes (poison_fill).
#include "../../include/abc_hip.h"

#include "abc_context.hpp"

namespace abc {

static bool capturing(abc_hip_ctx *c) {  // also sees a capture the caller began on its own stream
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(c->stream, &st) != hipSuccess) return false;
  return st != hipStreamCaptureStatusNone;
}
static void free_all(const std::vector<void *> &ptrs) {
  for (void *p : ptrs) (void)hipFree(p);
}

// ---- caching allocator --------------------------------------------------------------------------------------------------
// A freed buffer goes to a per-context free list (exact-size buckets) instead of back to the driver, and the next request of
// that size takes it -- no hipMalloc, no hipFree, no device synchronisation.  That is safe because every use of a context's
// buffers is ordered on the context's stream (the internal lanes fork from and join it inside each call, also on error paths:
// LaneScope): whatever still runs on a recycled buffer was issued before its new owner's first use.  A buffer handed to ANOTHER
// context or stream is the caller's to order (header).  It matters to the plugin classes, where the interpreter clones / drops
// a ciphertext on every variable read.  Two host threads may share a context for allocation (alloc_mu); the cache is flushed by
// abc_hip_trim, when the cap is reached, and whenever a hipMalloc of this context fails.
// (hipMallocAsync / hipFreeAsync were tried first and returned wrong results on some boxes of this pool when two contexts
// alternated -- analysis in DESIGN.md section 4b; ABC_HIP_SYNC_ALLOC=1 turns the cache off.)
// ABC_HIP_POISON=1 (debug): every block handed out -- a cache hit and a fresh hipMalloc alike -- and the scratch arenas, when they
// grow and when an outermost C-ABI operation begins, are filled with 0xFF bytes on the context's stream, so that a kernel which
// leaves output unwritten or reads scratch it never wrote cannot find a previous call's words there.  Nothing is filled while a
// capture is open (a recording gains no memset node), and keys and key mirrors are never filled.

static int poison_fill(abc_hip_ctx *c, void *p, size_t bytes) {
  if (!c->poison || !p || !bytes || c->buffers.capturing || capturing(c)) return 0;
  ABC_HIP_CHECK(hipMemsetAsync(p, 0xFF, bytes, c->stream));
  return 0;
}
void poison_arenas(abc_hip_ctx *c) {
  (void)poison_fill(c, c->ws, c->ws_bytes);
  for (int i = 0; i < 7; i++) (void)poison_fill(c, c->aux[i], c->aux_bytes[i]);
}

// Give every cached block back to the driver.  The stream is drained first: a cached block may still be read by work that was
// enqueued before it was freed.
int trim_cache(abc_hip_ctx *c) {
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  if (!c->buffers.cached_bytes()) return 0;
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  free_all(c->buffers.trim());
  return 0;
}
// hipMalloc; on failure flush this context's cache once and try again (the cache never shrinks by itself)
static hipError_t malloc_retry(abc_hip_ctx *c, void **p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return e;
  (void)hipGetLastError();
  if (trim_cache(c)) return e;
  return hipMalloc(p, bytes);
}

int buffer_malloc(abc_hip_ctx *c, void **d_ptr, size_t bytes) {
  if (!bytes) bytes = 8;
  if (c->cache_alloc) {
    std::lock_guard<std::mutex> lock(c->alloc_mu);
    const BufferTable::Take t = c->buffers.take(bytes, d_ptr);
    if (t == BufferTable::Take::hit) return poison_fill(c, *d_ptr, bytes);
    if (t == BufferTable::Take::refused) {
      set_error("allocation during graph capture found no cached buffer: run the sequence once eagerly first");
      return 1;
    }
  }
  ABC_HIP_CHECK(malloc_retry(c, d_ptr, bytes));
  if (c->cache_alloc) {
    std::lock_guard<std::mutex> lock(c->alloc_mu);
    c->buffers.add_block(*d_ptr, bytes);
  }
  return poison_fill(c, *d_ptr, bytes);
}
int buffer_free(abc_hip_ctx *c, void *d_ptr) {
  if (!d_ptr) return 0;
  if (c->cache_alloc) {
    BufferTable::Release r;
    {
      std::lock_guard<std::mutex> lock(c->alloc_mu);
      r = c->buffers.release(d_ptr);
    }
    if (r == BufferTable::Release::cached || r == BufferTable::Release::parked) return 0;
    if (r == BufferTable::Release::over_cap && trim_cache(c)) return 1;
  }
  NOT_CAPTURABLE(c, "abc_hip_free of an uncached buffer");
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  ABC_HIP_CHECK(hipFree(d_ptr));
  return 0;
}
size_t cached_bytes(abc_hip_ctx *c) {
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  return c->buffers.cached_bytes();
}
int held_buffers(const abc_hip_ctx *c) {
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  return (int)c->buffers.held();
}
void free_buffers(abc_hip_ctx *c) {
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  free_all(c->buffers.drain());
}

// ---- context buffers ----------------------------------------------------------------------------------------------------
hipError_t alloc_context_buffer(abc_hip_ctx *c, void **p, size_t bytes, bool retry) {
  const hipError_t e = retry ? malloc_retry(c, p, bytes) : hipMalloc(p, bytes);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  c->buffers.add_context_buffer(*p, bytes);
  return e;
}
void retire_buffer(abc_hip_ctx *c, void *p) {
  if (!p) return;
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  if (c->buffers.retire(p)) (void)hipFree(p);
}

static int ensure_arena(abc_hip_ctx *c, void **buf, size_t *have, size_t bytes, size_t headroom) {
  if (bytes <= *have) return 0;
  if (capturing(c)) { set_error("scratch would grow during graph capture: run the sequence once eagerly first"); return 1; }
  if (*buf) {
    ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
    retire_buffer(c, *buf);
    *buf = nullptr;
    *have = 0;
  }
  ABC_HIP_CHECK(alloc_context_buffer(c, buf, bytes + headroom, true));
  *have = bytes + headroom;
  return poison_fill(c, *buf, *have);
}
int ensure_workspace(abc_hip_ctx *c, size_t bytes) { return ensure_arena(c, &c->ws, &c->ws_bytes, bytes, bytes / 8); }
int ensure_aux(abc_hip_ctx *c, int which, size_t bytes) { return ensure_arena(c, &c->aux[which], &c->aux_bytes[which], bytes, 0); }

// ---- recorded circuits --------------------------------------------------------------------------------------------------
int graph_begin(abc_hip_ctx *c) {
  ABC_HIP_CHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  c->buffers.begin_capture();
  return 0;
}
int graph_end(abc_hip_ctx *c, void **out) {
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(c->stream, &graph);
  hipGraphExec_t exec = nullptr;
  if (e == hipSuccess) {
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
  }
  if (e != hipSuccess) (void)hipGetLastError();
  {
    std::lock_guard<std::mutex> lock(c->alloc_mu);
    free_all(c->buffers.end_capture(e == hipSuccess ? (void *)exec : nullptr));  // abandoned: its pins are let go
  }
  if (e != hipSuccess) {
    set_error(std::string("graph capture failed: ") + hipGetErrorString(e));
    return 1;
  }
  *out = exec;
  return 0;
}
int graph_destroy(abc_hip_ctx *c, void *exec) {
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  ABC_HIP_CHECK(hipGraphExecDestroy((hipGraphExec_t)exec));
  // what the caller had already freed goes back to the cache now; arenas and keys held back for this graph alone are freed
  // (the stream is drained above)
  std::lock_guard<std::mutex> lock(c->alloc_mu);
  free_all(c->buffers.drop_owner(exec));
  return 0;
}

// ---- mirrors of key-switching keys ---------------------------------------------------------------------------------------
// fp64 twin.  The split kernels multiply every key word into an fp64 residue: as u64 it costs a conversion per use (two
// instructions, sixteen words per thread of the last step); as a centred double, converted once when the key is first used,
// nothing.  Same layout [digit][2][K][N]; words modulo primes above 2^52 convert inexactly and are never read (the fp64 kernels
// touch fp64-capable primes only).
__global__ __launch_bounds__(256) void k_key_to_fp(DevCtx c, const u64 *__restrict__ key, double *__restrict__ keyf, size_t words) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const int kp = (int)((i >> c.logn) % (size_t)c.K);
    const u64 q = c.mods[kp].q, v = key[i];
    keyf[i] = v > (q >> 1) ? -(double)(q - v) : (double)v;
  }
}
// Shoup quotients, floor(w 2^64 / q) per word, same layout: with them a term of the inner product is one lazy Shoup product of
// ANY 64-bit transform output (no canonicalisation, no 128-bit product, no Barrett).
__global__ __launch_bounds__(256) void k_key_to_shoup(DevCtx c, const u64 *__restrict__ key, u64 *__restrict__ ks, size_t words) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const int kp = (int)((i >> c.logn) % (size_t)c.K);
    const u64 q = c.mods[kp].q;
    u64 r = key[i], quo = 0;  // r < q < 2^61: schoolbook division of r 2^64 by q, one quotient bit per step
    for (int bit = 0; bit < 64; bit++) {
      r <<= 1;
      const bool ge = r >= q;
      r -= ge ? q : 0;
      quo = (quo << 1) | (ge ? 1u : 0u);
    }
    ks[i] = quo;
  }
}
template <class T>
static void fill_mirror(abc_hip_ctx *c, void (*kernel)(DevCtx, const u64 *, T *, size_t), const u64 *key, T *d) {
  const size_t words = c->key_words();
  hipLaunchKernelGGL(kernel, dim3(grid_for(words, 256)), dim3(256), 0, c->stream, c->dc, key, d, words);
}
// Built on first use, on c->stream (so BEFORE fork_lanes: the lanes wait for an event recorded behind it), never inside a
// capture: the eager pass that precedes every recording builds it.  nullptr: not available.
template <class T>
static const T *mirror(abc_hip_ctx *c, const u64 *key, T *abc_hip_ctx::KeyMirror::*which,
                       void (*kernel)(DevCtx, const u64 *, T *, size_t)) {
  if (c->sw.no_key_twin || !key) return nullptr;
  auto it = c->key_mirrors.find(key);
  if (it != c->key_mirrors.end() && it->second.*which) return it->second.*which;
  if (c->buffers.capturing) return nullptr;
  T *d = nullptr;
  if (alloc_context_buffer(c, (void **)&d, c->key_words() * 8, false) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  fill_mirror(c, kernel, key, d);
  c->key_mirrors[key].*which = d;
  return d;
}
const double *key_twin(abc_hip_ctx *c, const u64 *key) { return mirror(c, key, &abc_hip_ctx::KeyMirror::twin, k_key_to_fp); }
const u64 *key_shoup(abc_hip_ctx *c, const u64 *key) { return mirror(c, key, &abc_hip_ctx::KeyMirror::shoup, k_key_to_shoup); }
const double *key_twin_lookup(const abc_hip_ctx *c, const u64 *key) {  // no building: safe after the lanes have forked
  if (c->sw.no_key_twin) return nullptr;
  auto it = c->key_mirrors.find(key);
  return it == c->key_mirrors.end() ? nullptr : it->second.twin;
}
// The permuted key of a hoisted rotation: an index permutation of every row (k_galois in NTT form over the L * 2 polynomials of K
// limbs).  Not subject to no_key_twin: without it the hoisted form has no key to switch with.
static int fill_permuted(abc_hip_ctx *c, const u64 *key, u64 *perm, u32 ginv) {
  return launch_galois(c, key, perm, c->K, (size_t)c->L * 2, ginv, true);
}
const u64 *key_permuted(abc_hip_ctx *c, const u64 *key, u32 ginv) {
  auto it = c->key_mirrors.find(key);
  if (it != c->key_mirrors.end() && it->second.perm) return it->second.perm;
  if (c->buffers.capturing) { set_error("permuted Galois key not built during graph capture: run the sequence once eagerly first"); return nullptr; }
  u64 *d = nullptr;
  if (alloc_context_buffer(c, (void **)&d, c->key_words() * 8, true) != hipSuccess) {
    (void)hipGetLastError();
    set_error("no device memory for the permuted Galois key");
    return nullptr;
  }
  if (fill_permuted(c, key, d, ginv)) { retire_buffer(c, d); return nullptr; }
  abc_hip_ctx::KeyMirror &m = c->key_mirrors[key];
  m.perm = d;
  m.perm_ginv = ginv;
  return d;
}
int refresh_key_mirrors(abc_hip_ctx *c, const u64 *key) {
  // the permuted keys first: they are keys with twins of their own, filled from them in the second pass (one stream: in order)
  const u64 *perm_of_key = nullptr;
  for (auto &kv : c->key_mirrors)
    if ((!key || kv.first == key) && kv.second.perm) {
      if (fill_permuted(c, kv.first, kv.second.perm, kv.second.perm_ginv)) return 1;  // a stale permuted key must not go unseen
      if (key) perm_of_key = kv.second.perm;
    }
  for (auto &kv : c->key_mirrors)  // whatever the switches say now: a recorded circuit may read the mirrors
    if (!key || kv.first == key || kv.first == perm_of_key) {
      if (kv.second.twin) fill_mirror(c, k_key_to_fp, kv.first, kv.second.twin);
      if (kv.second.shoup) fill_mirror(c, k_key_to_shoup, kv.first, kv.second.shoup);
    }
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
void release_key(abc_hip_ctx *c, u64 *key) {
  auto it = c->key_mirrors.find(key);
  if (it != c->key_mirrors.end()) {
    u64 *perm = it->second.perm;
    retire_buffer(c, it->second.twin);
    retire_buffer(c, it->second.shoup);
    c->key_mirrors.erase(it);
    if (perm) release_key(c, perm);  // and the mirrors of the permuted key
  }
  retire_buffer(c, key);
}

}  // namespace abc
