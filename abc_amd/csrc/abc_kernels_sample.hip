// abc_kernels_sample.hip -- the keyed sampling spec (abc_sample.hpp) on the device.
//
// Replaces the host draws behind seal::Encryptor::encrypt and seal::KeyGenerator for the OS-keyed entry points
// (src/runtime/SealCiphertextFactory.cpp:12, :89-93): one thread computes one ChaCha20 block and stores what the block yields,
// eight small coefficients (one 8-byte store) or four uniform residues (32 bytes).  No LDS, no cross-lane traffic; the key and
// the nonce are read from a 64-byte device buffer through scalar loads, never from the kernel arguments.
#include <cstring>

#include "abc_context.hpp"
#include "abc_sample.hpp"

namespace abc {

// ALU-bound, no memory latency to hide: four waves per SIMD on 256 CUs, the grid-stride loop beyond
static unsigned sample_grid(size_t threads) {
  const size_t g = (threads + 255) / 256, cap = 1024;
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}

struct SampleKey {
  uint32_t key[8];
  uint64_t stream;
};
__device__ __forceinline__ SampleKey load_sample_key(const u32 *kb, u64 stream_off) {
  const ABC_CONST_AS u32 *p = (const ABC_CONST_AS u32 *)kb;
  SampleKey k;
#pragma unroll
  for (int i = 0; i < 8; i++) k.key[i] = p[i];
  k.stream = ((u64)p[8] | ((u64)p[9] << 32)) + stream_off;
  return k;
}

// out: int8 [streams][polys][N]; stream s has id nonce + stream_off + s (mod 2^64) and polynomial p of it takes words
// p*N .. p*N + N - 1, the first `ternaries` polynomials ternary, the rest centred binomial.  One thread: one block.
// encryption: (count, 3, 1); secret key: (1, 1, 1); the errors of a key: (1, nkeys, 0).
__global__ __launch_bounds__(256) void k_sample_small(const u32 *__restrict__ kb, u64 stream_off, int logn, u32 polys, u32 ternaries,
                                                      size_t blocks, u64 *__restrict__ out) {
  const SampleKey k = load_sample_key(kb, stream_off);
  const int lb = logn - 3;  // blocks per polynomial: N is a multiple of 8, so a block never straddles two
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += stride) {
    const u32 poly = (u32)(b >> lb);  // over all streams
    const u32 s = poly / polys, p = poly - s * polys;
    u64 w[8];
    keyed::block(k.key, ((u64)p << lb) | (b & (((size_t)1 << lb) - 1)), k.stream + s, w);
    out[b] = keyed::pack_small(w, p < ternaries);
  }
}

// a: u64 [nkeys][K][N]; a_i[j][x] = (hi * 2^64 + lo) mod q_j from words 2t (lo), 2t + 1 (hi), t = (i*K + j)*N + x: block t / 4 holds
// four coefficients of one limb.  The wide reduction: ((hi mod q) * (2^64 mod q) + (lo mod q)) mod q.
__global__ __launch_bounds__(256) void k_sample_uniform(DevCtx c, const u32 *__restrict__ kb, u64 stream_off, size_t blocks,
                                                        u64 *__restrict__ a) {
  const SampleKey k = load_sample_key(kb, stream_off);
  const int lb = c.logn - 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += stride) {
    const Mod m = c.mods[(u32)(b >> lb) % (u32)c.K];
    const u64 r64 = reduce64(0 - m.q, m);  // 2^64 mod q
    u64 w[8];
    keyed::block(k.key, b, k.stream, w);
    u64x2 v[2];
    v[0].x = add_mod(mul_mod(reduce64(w[1], m), r64, m), reduce64(w[0], m), m.q);
    v[0].y = add_mod(mul_mod(reduce64(w[3], m), r64, m), reduce64(w[2], m), m.q);
    v[1].x = add_mod(mul_mod(reduce64(w[5], m), r64, m), reduce64(w[4], m), m.q);
    v[1].y = add_mod(mul_mod(reduce64(w[7], m), r64, m), reduce64(w[6], m), m.q);
    u64x2 *dst = reinterpret_cast<u64x2 *>(a + 4 * b);
    dst[0] = v[0];
    dst[1] = v[1];
  }
}

// key and nonce into the 64-byte device buffer d_kb; the host copy is wiped once the upload has completed
int upload_sample_key(abc_hip_ctx *c, void *d_kb, const uint8_t key[32], uint64_t nonce) {
  uint32_t h[kSampleKeyBytes / 4] = {};
  keyed::load_key(key, h);
  h[8] = (uint32_t)nonce;
  h[9] = (uint32_t)(nonce >> 32);
  const hipError_t e = hipMemcpyAsync(d_kb, h, sizeof(h), hipMemcpyHostToDevice, c->stream);
  const hipError_t s = hipStreamSynchronize(c->stream);
  explicit_bzero(h, sizeof(h));
  ABC_HIP_CHECK(e);
  ABC_HIP_CHECK(s);
  return 0;
}

int launch_sample_small(abc_hip_ctx *c, const void *d_kb, uint64_t stream_off, size_t streams, size_t polys, size_t ternaries,
                        int8_t *d_out) {
  const size_t total_polys = streams * polys;
  if (!total_polys) return 0;
  if (total_polys > 0xffffffffu) { set_error("sampling: batch too large for one call"); return 1; }
  const size_t blocks = total_polys << (c->logn - 3);
  hipLaunchKernelGGL(k_sample_small, dim3(sample_grid(blocks)), dim3(256), 0, c->stream, (const u32 *)d_kb, stream_off, c->logn, (u32)polys,
                     (u32)ternaries, blocks, (u64 *)d_out);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_sample_uniform(abc_hip_ctx *c, const void *d_kb, uint64_t stream_off, int nkeys, u64 *d_a) {
  const size_t blocks = ((size_t)nkeys * c->K) << (c->logn - 2);
  hipLaunchKernelGGL(k_sample_uniform, dim3(sample_grid(blocks)), dim3(256), 0, c->stream, c->dc, (const u32 *)d_kb, stream_off, blocks, d_a);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace abc
