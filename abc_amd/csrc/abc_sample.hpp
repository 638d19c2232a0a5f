// abc_sample.hpp -- the "keyed" sampling spec ("Keyed sampling spec"): counter-based ChaCha20 draws.
//
// Every 64-byte block is a pure function of (key, stream id, block number) and every coefficient depends on its own words only
// (no rejection loops), so the same functions serve one GPU thread per block (abc_kernels_sample.hip) and the host twin below.
// Plain C++17 outside hipcc: no HIP header, so the host twin compiles into a stand-alone (sanitised) test program too.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ABC_SAMPLE_FN __host__ __device__ __forceinline__
#define ABC_SAMPLE_UNROLL _Pragma("unroll")
#else
#define ABC_SAMPLE_FN inline
#define ABC_SAMPLE_UNROLL
#endif

namespace abc {
namespace keyed {

// stream ids of key generation (encryption: nonce + ciphertext index)
constexpr uint64_t kStreamSecret = 0, kStreamPublic = 1, kStreamRelin = 2;
constexpr uint64_t galois_stream(uint32_t elt) { return 2 + (uint64_t)elt; }  // elements are odd: no collision with 0 .. 2

ABC_SAMPLE_FN uint32_t rotl32(uint32_t v, int k) { return (v << k) | (v >> (32 - k)); }
ABC_SAMPLE_FN void quarter_round(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
  a += b; d ^= a; d = rotl32(d, 16);
  c += d; b ^= c; b = rotl32(b, 12);
  a += b; d ^= a; d = rotl32(d, 8);
  c += d; b ^= c; b = rotl32(b, 7);
}

// RFC 8439 block function; state words 12-13: 64-bit block counter, 14-15: 64-bit stream id (low word first).
// w[k] = out[2k] | out[2k+1] << 32: word number W of a stream is word W mod 8 of block W div 8.
ABC_SAMPLE_FN void block(const uint32_t key[8], uint64_t counter, uint64_t stream, uint64_t w[8]) {
  const uint32_t s4 = key[0], s5 = key[1], s6 = key[2], s7 = key[3], s8 = key[4], s9 = key[5], s10 = key[6], s11 = key[7];
  const uint32_t s12 = (uint32_t)counter, s13 = (uint32_t)(counter >> 32), s14 = (uint32_t)stream, s15 = (uint32_t)(stream >> 32);
  uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
  uint32_t x4 = s4, x5 = s5, x6 = s6, x7 = s7, x8 = s8, x9 = s9, x10 = s10, x11 = s11, x12 = s12, x13 = s13, x14 = s14, x15 = s15;
  ABC_SAMPLE_UNROLL
  for (int r = 0; r < 10; r++) {
    quarter_round(x0, x4, x8, x12); quarter_round(x1, x5, x9, x13); quarter_round(x2, x6, x10, x14); quarter_round(x3, x7, x11, x15);
    quarter_round(x0, x5, x10, x15); quarter_round(x1, x6, x11, x12); quarter_round(x2, x7, x8, x13); quarter_round(x3, x4, x9, x14);
  }
  w[0] = (uint64_t)(x0 + 0x61707865u) | ((uint64_t)(x1 + 0x3320646eu) << 32);
  w[1] = (uint64_t)(x2 + 0x79622d32u) | ((uint64_t)(x3 + 0x6b206574u) << 32);
  w[2] = (uint64_t)(x4 + s4) | ((uint64_t)(x5 + s5) << 32);
  w[3] = (uint64_t)(x6 + s6) | ((uint64_t)(x7 + s7) << 32);
  w[4] = (uint64_t)(x8 + s8) | ((uint64_t)(x9 + s9) << 32);
  w[5] = (uint64_t)(x10 + s10) | ((uint64_t)(x11 + s11) << 32);
  w[6] = (uint64_t)(x12 + s12) | ((uint64_t)(x13 + s13) << 32);
  w[7] = (uint64_t)(x14 + s14) | ((uint64_t)(x15 + s15) << 32);
}

// (w mod 3) - 1; 2^32 = 1 (mod 3), so the two halves may be added first (their sum, carry folded in, fits 32 bits)
ABC_SAMPLE_FN int ternary(uint64_t w) {
  const uint64_t s = (w & 0xffffffffu) + (w >> 32);
  return (int)(((uint32_t)s + (uint32_t)(s >> 32)) % 3u) - 1;
}
ABC_SAMPLE_FN int popcount21(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc((unsigned)v & 0x1FFFFFu);
#else
  return __builtin_popcount((unsigned)v & 0x1FFFFFu);
#endif
}
ABC_SAMPLE_FN int cbd(uint64_t w) { return popcount21(w) - popcount21(w >> 21); }

// eight consecutive coefficients (one block) of a small polynomial, packed as eight int8 in one 64-bit word, lowest byte first
ABC_SAMPLE_FN uint64_t pack_small(const uint64_t w[8], bool tern) {
  uint64_t packed = 0;
  ABC_SAMPLE_UNROLL
  for (int k = 0; k < 8; k++) packed |= (uint64_t)(uint8_t)(int8_t)(tern ? ternary(w[k]) : cbd(w[k])) << (8 * k);
  return packed;
}

// ---- host twin ----
inline void load_key(const uint8_t key[32], uint32_t out[8]) {
  for (int i = 0; i < 8; i++)
    out[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) | ((uint32_t)key[4 * i + 3] << 24);
}
inline uint64_t uniform_q(uint64_t lo, uint64_t hi, uint64_t q) { return (uint64_t)(((((unsigned __int128)hi) << 64) | lo) % q); }

// `polys` polynomials of n coefficients from one stream, polynomial p from words p*n .. p*n + n - 1; the first `ternaries`
// of them ternary, the rest centred binomial.  n is a multiple of 8.
inline void small_host(const uint32_t key[8], uint64_t stream, size_t n, size_t polys, size_t ternaries, int8_t *out) {
  uint64_t w[8];
  for (size_t b = 0; b < polys * n / 8; b++) {
    block(key, b, stream, w);
    const bool tern = b * 8 / n < ternaries;
    for (int k = 0; k < 8; k++) out[b * 8 + k] = (int8_t)(tern ? ternary(w[k]) : cbd(w[k]));
  }
}
// the draws of `count` ciphertexts, [count][3][n] (u | e0 | e1), ciphertext i from stream nonce + i (mod 2^64)
inline void encrypt_small_host(const uint8_t key[32], uint64_t nonce, size_t n, size_t count, int8_t *out) {
  uint32_t k[8];
  load_key(key, k);
  for (size_t i = 0; i < count; i++) small_host(k, nonce + i, n, 3, 1, out + i * 3 * n);
  for (volatile uint32_t &v : k) v = 0;
}
// a [nkeys][K][n]: a_i[j][x] from words 2t, 2t + 1, t = (i*K + j)*n + x, reduced modulo primes[j]
inline void uniform_host(const uint32_t key[8], uint64_t stream, size_t n, int K, const uint64_t *primes, int nkeys, uint64_t *a) {
  uint64_t w[8];
  for (size_t b = 0; b < (size_t)nkeys * K * n / 4; b++) {
    block(key, b, stream, w);
    const uint64_t q = primes[(b * 4 / n) % (size_t)K];
    for (int k = 0; k < 4; k++) a[b * 4 + k] = uniform_q(w[2 * k], w[2 * k + 1], q);
  }
}

}  // namespace keyed
}  // namespace abc
