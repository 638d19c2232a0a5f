// abc_crt_lift.hpp -- exact centred lift of an RNS residue vector into a multi-word integer, shared by the CKKS decoder
// (abc_kernels_ckks_codec.hip, SrcLift) and the BFV noise budget (abc_keys.hip, k_noise_bits).
//
// Garner digits d_j (value = d_0 + q_0 (d_1 + q_1 (d_2 + ...))), a multi-word Horner from the top digit, the compare with
// floor(Q / 2) of the level and the conditional Q - x: the magnitude of the representative in (-Q/2, Q/2] (Q odd: no tie) and its
// sign.  Integers only.  The per-context constants (CodecConst) are built on the host on first use, for either scheme.
#pragma once

#include "abc_context.hpp"
#include "abc_host_math.hpp"

namespace abc {

constexpr int kWords = kMaxLimbs;  // Q = q_0 ... q_{nl-1} < 2^(61 nl) fits nl words

// CRT constants of the lift (uploaded once per context)
struct CodecConst {
  u64 rad[kMaxLimbs][kMaxLimbs];  // [j][i] = q_0 ... q_{i-1} mod q_j   (i < j)
  u64 inv_rad[kMaxLimbs];         // (q_0 ... q_{j-1})^-1 mod q_j
  u64 Q[kMaxLimbs][kWords];       // [nl-1]: q_0 ... q_{nl-1}, little-endian words
  u64 Qh[kMaxLimbs][kWords];      // [nl-1]: floor(Q / 2)
};

// the context's CodecConst in device memory (abc_hip_ctx::d_crt), built and uploaded on first use
inline int ensure_crt_const(abc_hip_ctx *c) {
  if (c->d_crt) return 0;
  using namespace host;
  std::vector<char> blk(sizeof(CodecConst), 0);
  CodecConst *k = (CodecConst *)blk.data();
  uint64_t Q[kWords] = {1};
  for (int j = 0; j < c->L; ++j) {
    const uint64_t qj = c->primes[j];
    uint64_t rad = 1;
    for (int i = 0; i < j; ++i) {
      k->rad[j][i] = rad;
      rad = mulmod(rad, c->primes[i] % qj, qj);
    }
    k->inv_rad[j] = invmod(rad, qj);
    u128 carry = 0;
    for (int w = 0; w < kWords; ++w) {
      const u128 p = (u128)Q[w] * qj + carry;
      Q[w] = (uint64_t)p;
      carry = p >> 64;
    }
    for (int w = 0; w < kWords; ++w) {
      k->Q[j][w] = Q[w];
      k->Qh[j][w] = (Q[w] >> 1) | (w + 1 < kWords ? Q[w + 1] << 63 : 0);
    }
  }
  void *d = nullptr;
  ABC_HIP_CHECK(hipMalloc(&d, blk.size()));
  if (hipMemcpy(d, blk.data(), blk.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    set_error("CRT lift: table upload failed");
    return 1;
  }
  c->d_crt = d;
  return 0;
}

// x[0 .. NLW-1] (little-endian words) <- |v|, v the representative in (-Q/2, Q/2] of the value whose residue modulo q_j is
// res(j, m_j), j < nl <= NLW (m_j: the constants of q_j), Q = q_0 ... q_{nl-1}; returns true where v is negative.  mods: DevCtx::mods (data prime j is modulus j).
template <int NLW, class Res>
__device__ __forceinline__ bool crt_lift_centred(const Mod *mods, const CodecConst *k, int nl, Res res, u64 (&x)[NLW]) {
  // vector loads of the Garner and modulus constants (pointers moved to VGPRs): through the scalar unit the compiler hoists
  // all of them out of the caller's element loop and spills SGPRs
  asm volatile("" : "+v"(k), "+v"(mods));
  const CodecConst &kc = *k;
  u64 d[NLW];
#pragma unroll
  for (int j = 0; j < NLW; ++j) {  // Garner digits: value = d_0 + q_0 (d_1 + q_1 (d_2 + ...))
    d[j] = 0;
    if (j < nl) {
      const Mod m = mods[j];
      u64 acc = 0;
#pragma unroll
      for (int i = 0; i < j; ++i) acc = add_mod(acc, mul_mod(d[i], kc.rad[j][i], m), m.q);  // d_i < 2^61: one Barrett
      d[j] = mul_mod(sub_mod(res(j, m), acc, m.q), kc.inv_rad[j], m);
    }
  }
#pragma unroll
  for (int w = 0; w < NLW; ++w) x[w] = 0;
#pragma unroll
  for (int j = NLW - 1; j >= 0; --j) {  // Horner from the top digit: x < q_j ... q_{nl-1} fits nl - j words
    if (j < nl) {
      const u64 q = mods[j].q;
      u64 carry = d[j];
#pragma unroll
      for (int w = 0; w < NLW - j; ++w) {
        const u64 lo = x[w] * q, hi = mulhi64(x[w], q), s = lo + carry;
        carry = hi + (s < lo ? 1ull : 0ull);
        x[w] = s;
      }
    }
  }
  const u64 *Q = kc.Q[nl - 1], *Qh = kc.Qh[nl - 1];
  bool gt = false, decided = false;
#pragma unroll
  for (int w = NLW - 1; w >= 0; --w) {
    const u64 h = Qh[w];
    if (!decided && x[w] != h) {
      gt = x[w] > h;
      decided = true;
    }
  }
  if (gt) {  // x > Q/2: the value is x - Q; take Q - x and negate
    u64 borrow = 0;
#pragma unroll
    for (int w = 0; w < NLW; ++w) {
      const u64 a = Q[w], t = a - x[w];
      const u64 nb = (a < x[w] || t < borrow) ? 1ull : 0ull;
      x[w] = t - borrow;
      borrow = nb;
    }
  }
  return gt;
}

}  // namespace abc
