// abc_kernels_eval.hip -- evaluator kernels shared by BFV and CKKS (generic, any N = 2^10..2^16):
// limb-wise add/sub/negate, CKKS dyadic tensor, hybrid key switching with one special prime,
// Galois automorphisms, rescale / modulus drop.
//
// Reference call sites replaced (src/runtime/SealCiphertext.cpp): add :92,:114; sub :98,:118;
// negate :157,:193; relinearize_inplace :105,:123,:160,:197; rotate_rows :55,:60.
// Key switching follows seal::Evaluator::switch_key_inplace: decomposition limb J is reduced modulo
// every key-level prime, transformed, multiplied with key[J] and accumulated; the special-prime limb is
// then divided out with rounding.  All outputs are fully reduced, hence bit-comparable with oracle/.
// That division and rescale's are one piece of mathematics (abc_ntt.hpp, "divide by a dropped prime"): the generic pair
// k_divround_tmod / k_divround_finish serves both, and rescale's LDS-resident kernels call the bodies the key switch's mod-down
// calls (divround_to_coef, divround_finish).
#include <cstdlib>

#include "abc_context.hpp"

namespace abc {

LimbMap key_limb_map(const abc_hip_ctx *c, int nl) {
  LimbMap m{};
  for (int j = 0; j < nl; j++) m.id[j] = j;
  m.id[nl] = c->K - 1;
  return m;
}

// ---- limb-wise add / sub / negate:  data viewed as [polys][nl][N] ----
__global__ __launch_bounds__(256) void k_addsub(DevCtx c, const u64 *a, const u64 *b, u64 *out, int nl, size_t words, int op) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 2;
  for (size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; w < words; w += stride) {
    const int j = (int)((w >> c.logn) % nl);
    const u64 q = c.mods[j].q;
    u64x2 x = *reinterpret_cast<const u64x2 *>(a + w);
    u64x2 r;
    if (op == 2) {
      r.x = neg_mod(x.x, q);
      r.y = neg_mod(x.y, q);
    } else {
      u64x2 y = *reinterpret_cast<const u64x2 *>(b + w);
      if (op == 0) { r.x = add_mod(x.x, y.x, q); r.y = add_mod(x.y, y.y, q); }
      else { r.x = sub_mod(x.x, y.x, q); r.y = sub_mod(x.y, y.y, q); }
    }
    *reinterpret_cast<u64x2 *>(out + w) = r;
  }
}

int launch_addsub(abc_hip_ctx *c, const u64 *a, const u64 *b, u64 *out, int nl, size_t polys, int op) {
  const size_t words = polys * nl * (size_t)c->n;
  if (!words) return 0;
  hipLaunchKernelGGL(k_addsub, dim3(grid_for(words / 2, 256)), dim3(256), 0, c->stream, c->dc, a, b, out, nl, words, op);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- CKKS tensor product: (a0,a1) x (b0,b1) -> (a0b0, a0b1+a1b0, a1b1), NTT form ----
__global__ __launch_bounds__(256) void k_ckks_tensor(DevCtx c, const u64 *a, const u64 *b, u64 *out3, int nl, size_t count) {
  const size_t pw = (size_t)nl * c.n;  // words per polynomial
  const size_t items = count * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ct = it / pw, w = it % pw;
    const Mod m = c.mods[w >> c.logn];
    const u64 *pa = a + ct * 2 * pw + w, *pb = b + ct * 2 * pw + w;
    const u64 a0 = pa[0], a1 = pa[pw], b0 = pb[0], b1 = pb[pw];
    u64 *po = out3 + ct * 3 * pw + w;
    po[0] = mul_mod(a0, b0, m);
    U128 acc = mul_wide(a0, b1);
    mac128(acc, a1, b0);
    po[pw] = barrett_reduce(acc, m);
    po[2 * pw] = mul_mod(a1, b1, m);
  }
}

int launch_ckks_tensor(abc_hip_ctx *c, const u64 *a, const u64 *b, u64 *out3, int nl, size_t count) {
  const size_t items = count * nl * (size_t)c->n;
  if (!items) return 0;
  hipLaunchKernelGGL(k_ckks_tensor, dim3(grid_for(items, 256)), dim3(256), 0, c->stream, c->dc, a, b, out3, nl, count);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- CKKS tensor sum: out3 (+)= sum over the launch's terms of a_k (x) b_k, the front of abc_hip_multiply_sum / mul_sum_relin ----
// A streaming kernel: one workgroup owns kTensorSumSpan consecutive coefficients of ONE limb of one ciphertext, so the modulus is
// workgroup-uniform (scalar), every lane moves 16 bytes per load and store, and a term's four loads are issued before the previous
// term's arithmetic.  The term pointers travel by value (no device-side table, no copy: the call stays capturable); the loop over
// them is unrolled, so the record is only ever indexed by constants and stays in scalar registers.  A call of more than
// kTensorSumTerms terms takes several launches; ACC: this launch adds to the canonical (c0, c1, c2) an earlier one left in out3.
// Results are exact modular sums in canonical form, whatever the order: bit-identical to k_ckks_tensor + k_addsub per term.
struct TensorSumTerms {
  const u64 *a[kTensorSumTerms], *b[kTensorSumTerms];
};
constexpr int kTensorSumSpan = 512;  // coefficients per workgroup: 256 lanes x u64x2; divides every ring (N >= 2^10)
// Integer limbs accumulate the 128-bit products lazily and reduce once per launch.  A launch sums at most 2 * kTensorSumTerms
// products into c1, plus the carried value (below q: less than one product): (2 T + 1) (q - 1)^2 < 2^128 must hold for the widest
// prime a context accepts, 2^60 (abc_hip_ctx_create) -- 2^(128 - 2 * 60) = 256 products, so T could be 127; the launch boundary is
// the intermediate reduction.  barrett_reduce itself wants x < 2^(k+63): reduce128 folds the high word first.
constexpr unsigned kTensorSumPrimeBits = kIsplitBits;  // 60: the widest data prime
static_assert(2 * kTensorSumTerms + 1 <= (1 << (128 - 2 * kTensorSumPrimeBits)), "tensor sum: the 128-bit accumulator would overflow within one launch");
// fp64 limbs (q < 2^50): products |.| < q (fp_mulmod) are summed as integer-valued doubles, exact below 2^53 > 8 q.  c1 takes two
// per term, so every accumulator is re-centred (|.| <= q/2) after kTensorSumFpTerms = 3 terms: the carried value (below q when it
// is the canonical word of an earlier launch, else <= q/2) plus six products stays below 7 q < 2^53.
constexpr int kTensorSumFpTerms = 3;
static_assert((2 * kTensorSumFpTerms + 1) <= 8, "tensor sum: the fp64 accumulator would pass 2^53 between two re-centrings");

// x (any 128-bit value) mod q: hi * 2^64 + lo = reduce64(hi) * r64 + lo (mod q), r64 = 2^64 mod q; the right side is below
// q^2 + 2^64 < 2^(k+63)
__device__ __forceinline__ u64 reduce128(const U128 &x, u64 r64, const Mod &m) {
  U128 t = mul_wide(reduce64(x.hi, m), r64);
  add128(t, U128{x.lo, 0});
  return barrett_reduce(t, m);
}

struct TensorSumLoad {
  u64x2 a0, a1, b0, b1;
};
__device__ __forceinline__ TensorSumLoad tensor_sum_load(const u64 *a, const u64 *b, size_t off, size_t pw) {
  TensorSumLoad t;
  t.a0 = *reinterpret_cast<const u64x2 *>(a + off);
  t.a1 = *reinterpret_cast<const u64x2 *>(a + off + pw);
  t.b0 = *reinterpret_cast<const u64x2 *>(b + off);
  t.b1 = *reinterpret_cast<const u64x2 *>(b + off + pw);
  return t;
}

// one tile on the integers
template <bool ACC>
__device__ __forceinline__ void tensor_sum_int(const TensorSumTerms &t, int nt, const Mod &m, size_t in_off, size_t pw, u64 *po) {
  U128 c0x{0, 0}, c0y{0, 0}, c1x{0, 0}, c1y{0, 0}, c2x{0, 0}, c2y{0, 0};
  if constexpr (ACC) {
    const u64x2 r0 = *reinterpret_cast<const u64x2 *>(po), r1 = *reinterpret_cast<const u64x2 *>(po + pw),
                r2 = *reinterpret_cast<const u64x2 *>(po + 2 * pw);
    c0x.lo = r0.x, c0y.lo = r0.y, c1x.lo = r1.x, c1y.lo = r1.y, c2x.lo = r2.x, c2y.lo = r2.y;
  }
  TensorSumLoad cur = tensor_sum_load(t.a[0], t.b[0], in_off, pw), nxt = cur;
#pragma unroll
  for (int k = 0; k < kTensorSumTerms; k++) {
    if (k < nt) {  // workgroup-uniform
      if (k + 1 < kTensorSumTerms && k + 1 < nt) nxt = tensor_sum_load(t.a[k + 1], t.b[k + 1], in_off, pw);
      mac128(c0x, cur.a0.x, cur.b0.x), mac128(c0y, cur.a0.y, cur.b0.y);
      mac128(c1x, cur.a0.x, cur.b1.x), mac128(c1y, cur.a0.y, cur.b1.y);
      mac128(c1x, cur.a1.x, cur.b0.x), mac128(c1y, cur.a1.y, cur.b0.y);
      mac128(c2x, cur.a1.x, cur.b1.x), mac128(c2y, cur.a1.y, cur.b1.y);
      cur = nxt;
    }
  }
  const u64 r64 = reduce64(0ull - m.q, m);  // 2^64 mod q
  *reinterpret_cast<u64x2 *>(po) = u64x2{reduce128(c0x, r64, m), reduce128(c0y, r64, m)};
  *reinterpret_cast<u64x2 *>(po + pw) = u64x2{reduce128(c1x, r64, m), reduce128(c1y, r64, m)};
  *reinterpret_cast<u64x2 *>(po + 2 * pw) = u64x2{reduce128(c2x, r64, m), reduce128(c2y, r64, m)};
}

// one tile in fp64 (q < 2^50)
template <bool ACC>
__device__ __forceinline__ void tensor_sum_fp(const TensorSumTerms &t, int nt, const Mod &m, size_t in_off, size_t pw, u64 *po) {
  const double q = m.qd, qinv = m.qinv;
  double c0x = 0, c0y = 0, c1x = 0, c1y = 0, c2x = 0, c2y = 0;
  if constexpr (ACC) {
    const u64x2 r0 = *reinterpret_cast<const u64x2 *>(po), r1 = *reinterpret_cast<const u64x2 *>(po + pw),
                r2 = *reinterpret_cast<const u64x2 *>(po + 2 * pw);
    c0x = fp_from_u64(r0.x), c0y = fp_from_u64(r0.y), c1x = fp_from_u64(r1.x), c1y = fp_from_u64(r1.y);
    c2x = fp_from_u64(r2.x), c2y = fp_from_u64(r2.y);
  }
  TensorSumLoad cur = tensor_sum_load(t.a[0], t.b[0], in_off, pw), nxt = cur;
#pragma unroll
  for (int k = 0; k < kTensorSumTerms; k++) {
    if (k < nt) {  // workgroup-uniform
      if (k + 1 < kTensorSumTerms && k + 1 < nt) nxt = tensor_sum_load(t.a[k + 1], t.b[k + 1], in_off, pw);
      const double a0x = fp_from_u64(cur.a0.x), a0y = fp_from_u64(cur.a0.y), a1x = fp_from_u64(cur.a1.x), a1y = fp_from_u64(cur.a1.y);
      const double b0x = fp_from_u64(cur.b0.x), b0y = fp_from_u64(cur.b0.y), b1x = fp_from_u64(cur.b1.x), b1y = fp_from_u64(cur.b1.y);
      c0x += fp_mulmod(a0x, b0x, q, qinv), c0y += fp_mulmod(a0y, b0y, q, qinv);
      c1x += fp_mulmod(a0x, b1x, q, qinv), c1y += fp_mulmod(a0y, b1y, q, qinv);
      c1x += fp_mulmod(a1x, b0x, q, qinv), c1y += fp_mulmod(a1y, b0y, q, qinv);
      c2x += fp_mulmod(a1x, b1x, q, qinv), c2y += fp_mulmod(a1y, b1y, q, qinv);
      // carried value + 2 * kTensorSumFpTerms products < 7 q < 2^53 up to here (see kTensorSumFpTerms); the last group of the
      // launch is centred by fp_to_canon
      if ((k + 1) % kTensorSumFpTerms == 0 && k + 1 < kTensorSumTerms) {
        c0x = fp_centre(c0x, q, qinv), c0y = fp_centre(c0y, q, qinv), c1x = fp_centre(c1x, q, qinv), c1y = fp_centre(c1y, q, qinv);
        c2x = fp_centre(c2x, q, qinv), c2y = fp_centre(c2y, q, qinv);
      }
      cur = nxt;
    }
  }
  *reinterpret_cast<u64x2 *>(po) = u64x2{fp_to_canon(c0x, q, qinv), fp_to_canon(c0y, q, qinv)};
  *reinterpret_cast<u64x2 *>(po + pw) = u64x2{fp_to_canon(c1x, q, qinv), fp_to_canon(c1y, q, qinv)};
  *reinterpret_cast<u64x2 *>(po + 2 * pw) = u64x2{fp_to_canon(c2x, q, qinv), fp_to_canon(c2y, q, qinv)};
}

// tiles = count * nl * (N / kTensorSumSpan), tile -> (ciphertext, limb, span) with scalar arithmetic; fpmask bit j: limb j in fp64.
// HAS_FP / HAS_INT: which arithmetic the chain's first nl limbs need (both: a mixed chain, a workgroup-uniform branch)
template <bool HAS_FP, bool HAS_INT, bool ACC>
__global__ __launch_bounds__(256) void k_ckks_tensor_sum(DevCtx c, TensorSumTerms t, int nt, u64 *out3, int nl, size_t tiles, u32 fpmask) {
  const u32 spans = (u32)c.n / kTensorSumSpan;
  const size_t pw = (size_t)nl * c.n;
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t limb = tile / spans;  // ct * nl + j
    const u32 span = (u32)(tile - limb * spans);
    const size_t ct = limb / (u32)nl;
    const int j = (int)(limb - ct * (u32)nl);
    const size_t w = (size_t)j * c.n + (size_t)span * kTensorSumSpan + 2 * threadIdx.x;  // word inside a polynomial
    const Mod m = mod_at(c, j);
    u64 *po = out3 + ct * 3 * pw + w;
    const size_t in_off = ct * 2 * pw + w;
    if (HAS_FP && (!HAS_INT || ((fpmask >> j) & 1u))) tensor_sum_fp<ACC>(t, nt, m, in_off, pw, po);
    else tensor_sum_int<ACC>(t, nt, m, in_off, pw, po);
  }
}

// out3 = sum over k < n_terms of a[k] (x) b[k]; n_terms >= 1 (the caller writes the zeros of an empty sum), on stream c->stream
int launch_ckks_tensor_sum(abc_hip_ctx *c, const u64 *const *a, const u64 *const *b, int n_terms, u64 *out3, int nl, size_t count) {
  const size_t tiles = count * nl * ((size_t)c->n / kTensorSumSpan);
  if (!tiles || n_terms < 1) return 0;
  const u32 full = (1u << nl) - 1u;
  const u32 fpmask = (c->use_fp && (c->facts.data_fp(nl) || !c->sw.no_mixed)) ? c->facts.fp_data_mask(nl) : 0u;
  const size_t cap = 256 * 8 * 16;  // workgroups: every CU several times over, the tile loop beyond
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
  for (int k0 = 0; k0 < n_terms; k0 += kTensorSumTerms) {
    const int nt = n_terms - k0 < kTensorSumTerms ? n_terms - k0 : kTensorSumTerms;
    TensorSumTerms t;
    for (int k = 0; k < kTensorSumTerms; k++) t.a[k] = a[k0 + (k < nt ? k : 0)], t.b[k] = b[k0 + (k < nt ? k : 0)];
    auto go = [&](auto has_fp, auto has_int, auto acc) {
      hipLaunchKernelGGL((k_ckks_tensor_sum<decltype(has_fp)::value, decltype(has_int)::value, decltype(acc)::value>), grid, dim3(256), 0,
                         c->stream, c->dc, t, nt, out3, nl, tiles, fpmask);
    };
    auto by_acc = [&](auto has_fp, auto has_int) {
      if (k0) go(has_fp, has_int, std::true_type{});
      else go(has_fp, has_int, std::false_type{});
    };
    if (fpmask == full) by_acc(std::true_type{}, std::false_type{});
    else if (!fpmask) by_acc(std::false_type{}, std::true_type{});
    else by_acc(std::true_type{}, std::true_type{});
    ABC_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// ---- key switching, generic path ----
// dec[ct][J][I][k] = tcoef[ct][J][k] mod q_{ki(I)}
__global__ __launch_bounds__(256) void k_ks_expand(DevCtx c, const u64 *tcoef, size_t tstride, u64 *dec, int nl, size_t count) {
  const size_t per_ct = (size_t)nl * c.n;
  const size_t items = count * per_ct;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ct = it / per_ct, r = it % per_ct;
    const int J = (int)(r >> c.logn);
    const size_t k = r & (c.n - 1);
    const u64 v = tcoef[ct * tstride + r];
    u64 *d = dec + ((ct * nl + J) * (size_t)(nl + 1)) * c.n + k;
    for (int I = 0; I <= nl; I++) {
      const int ki = (I == nl) ? c.K - 1 : I;
      d[(size_t)I * c.n] = reduce64(v, c.mods[ki]);
    }
  }
}

// prodD[ct][comp][I<nl][k], prodS[ct][comp][k] = sum_J dec[ct][J][I][k] * key[J][comp][ki][k]
__global__ __launch_bounds__(256) void k_ks_inner(DevCtx c, const u64 *dec, const u64 *key, u64 *prodD, u64 *prodS, int nl,
                                                  size_t count) {
  const size_t per_ct = (size_t)(nl + 1) * c.n;
  const size_t items = count * per_ct;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ct = it / per_ct, r = it % per_ct;
    const int I = (int)(r >> c.logn);
    const size_t k = r & (c.n - 1);
    const int ki = (I == nl) ? c.K - 1 : I;
    const Mod m = c.mods[ki];
    u64 acc0 = 0, acc1 = 0;
    for (int J = 0; J < nl; J++) {
      const u64 x = dec[((ct * nl + J) * (size_t)(nl + 1) + I) * c.n + k];
      const u64 *kj = key + (((size_t)J * 2) * c.K + ki) * c.n + k;
      acc0 = add_mod(acc0, mul_mod(x, kj[0], m), m.q);
      acc1 = add_mod(acc1, mul_mod(x, kj[(size_t)c.K * c.n], m), m.q);
    }
    if (I == nl) {
      prodS[(ct * 2 + 0) * c.n + k] = acc0;
      prodS[(ct * 2 + 1) * c.n + k] = acc1;
    } else {
      prodD[((ct * 2 + 0) * nl + I) * c.n + k] = acc0;
      prodD[((ct * 2 + 1) * nl + I) * c.n + k] = acc1;
    }
  }
}

// ---- divide by a dropped prime with rounding, one thread per coefficient (abc_ntt.hpp has the mathematics): the pair of kernels
// around the stand-alone transforms, for the key switch's special prime and for rescale's last limb ----
// tmod[poly][j < nrem][k] = ((last + half) mod p) mod q_j + fix(p, q_j),  p = prime `drop`, last = its limb in coefficient form
__global__ __launch_bounds__(256) void k_divround_tmod(DevCtx c, const u64 *last, u64 *tmod, int drop, int nrem, size_t polys) {
  const size_t items = polys * c.n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const Mod md = c.mods[drop];
  const u64 half = md.q >> 1;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t p = it >> c.logn, k = it & (c.n - 1);
    const u64 v = add_mod(last[it], half, md.q);
    for (int j = 0; j < nrem; j++) {
      const Mod m = c.mods[j];
      tmod[(p * nrem + j) * c.n + k] = add_mod(reduce64(v, m), round_fix(half, m), m.q);
    }
  }
}

// out[poly][j < nrem][k] = (in[poly][j] - tmod) * p^-1 mod q_j  (+ addend);  in: in_limbs limbs per polynomial; inv, inv_s: p^-1 mod
// q_j and its Shoup quotient (a row of DevConst); polynomials are (ct, comp) pairs where there is an addend
__global__ __launch_bounds__(256) void k_divround_finish(DevCtx c, const u64 *in, int in_limbs, const u64 *tmod, u64 *out, const u64 *inv,
                                                         const u64 *inv_s, const u64 *addend, size_t addend_stride, int add_c1, int nrem,
                                                         size_t polys) {
  const size_t items = polys * nrem * (size_t)c.n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t limb = it >> c.logn, k = it & (c.n - 1);
    const size_t p = limb / nrem;
    const int j = (int)(limb % nrem);
    const u64 q = c.mods[j].q;
    u64 v = mul_shoup(sub_mod(in[(p * in_limbs + j) * c.n + k], tmod[it], q), inv[j], inv_s[j], q);
    if (addend && ((p & 1) == 0 || add_c1)) v = add_mod(v, addend[(p >> 1) * addend_stride + ((p & 1) * nrem + j) * c.n + k], q);
    out[it] = v;
  }
}

static int launch_divround_tmod(abc_hip_ctx *c, const u64 *last, u64 *tmod, int drop, int nrem, size_t polys) {
  hipLaunchKernelGGL(k_divround_tmod, dim3(grid_for(polys * c->n, 256)), dim3(256), 0, c->stream, c->dc, last, tmod, drop, nrem, polys);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
static int launch_divround_finish(abc_hip_ctx *c, const u64 *in, int in_limbs, const u64 *tmod, u64 *out, const u64 *inv, const u64 *inv_s,
                                  const u64 *addend, size_t addend_stride, bool add_c1, int nrem, size_t polys) {
  hipLaunchKernelGGL(k_divround_finish, dim3(grid_for(polys * nrem * (size_t)c->n, 256)), dim3(256), 0, c->stream, c->dc, in, in_limbs,
                     tmod, out, inv, inv_s, addend, addend_stride, (int)add_c1, nrem, polys);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
// the key switch's: p = the special prime
int launch_ks_tmod(abc_hip_ctx *c, const u64 *prodS, u64 *tmod, int nl, size_t polys) {
  return launch_divround_tmod(c, prodS, tmod, c->K - 1, nl, polys);
}
int launch_ks_finish(abc_hip_ctx *c, const u64 *prodD, const u64 *tmod, u64 *out, const u64 *addend, size_t addend_stride,
                     bool add_c1, int nl, size_t count) {
  return launch_divround_finish(c, prodD, nl, tmod, out, c->dc.cst->inv_special, c->dc.cst->inv_special_s, addend, addend_stride, add_c1,
                                nl, count * 2);
}

// ---- N = 2^15 / 2^16, integer arithmetic (a key prime above 2^50: config 5's 55-bit chain): decomposition and inner product
// in two kernels instead of five.  The generic sequence writes every digit once per key prime (k_ks_expand), carries those
// nl (nl + 1) limbs through the strided pass and the block transforms (two round trips) and reads them again in k_ks_inner:
// five transfers of nl (nl + 1) limbs.  Here:
//   k_iks_pass0   (ct, digit J, key prime I, 256 positions): digit J read as it lies, reduced modulo q_I, strided first
//                 stages -> half-done limb (ct, J, I)                                        [one write]
//   k_iks_special (ct, key prime I, 4096-point block b): per digit J the block stages in LDS, the transform's outputs go
//                 straight from registers into the two inner products with the key (same register layout for every J and
//                 for the inverse block transform that follows), then the inverse block stages of both sums -> prodD /
//                 prodS half-done (the strided last stages, q_sp rounding and the subtraction stay with the generic
//                 kernels)                                                                    [one read, 2 / nl of a write]
// Inner products: canonical operands, one Barrett product per term (a 128-bit accumulator per value would cost 128 VGPRs).
template <int R>
__global__ __launch_bounds__(256) void k_iks_pass0(DevCtx c, const u64 *__restrict__ tcoef, size_t tstride, u64 *__restrict__ dec, int nl,
                                                   u32 ginv /* BFV rotation: elt^-1 mod 2N, the signed permutation folded into the load */) {
  const int G = c.n >> R;
  const int per = G / 256;
  const size_t limb = blockIdx.x / per;  // (ct * nl + J) * (nl + 1) + I
  const int p = (blockIdx.x % per) * 256 + threadIdx.x;
  const int I = (int)(limb % (size_t)(nl + 1));
  const size_t cj = limb / (size_t)(nl + 1);
  const int J = (int)(cj % (size_t)nl);
  const size_t ct = cj / (size_t)nl;
  const int ki = (I == nl) ? c.K - 1 : I;
  const Mod m = c.mods[ki];
  const NttTable t = ntt_table(c, ki);
  const u64 *__restrict__ src = tcoef + ct * tstride + (size_t)J * c.n + p;
  u64 x[1 << R];
  if (ginv) {  // workgroup-uniform
    const u64 *__restrict__ limb = tcoef + ct * tstride + (size_t)J * c.n;
    const u64 qj = c.mods[J].q;
#pragma unroll
    for (int k = 0; k < (1 << R); k++) {
      bool neg;
      const u64 v = limb[galois_coef_src((u32)(k * G + p), ginv, c.logn, neg)];
      x[k] = neg ? neg_mod(v, qj) : v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < (1 << R); k++) x[k] = src[(size_t)k * G];
  }
#pragma unroll
  for (int k = 0; k < (1 << R); k++) x[k] = reduce64(x[k], m);
#pragma unroll
  for (int u = 0; u < R; u++) {
    const int half = 1 << (R - 1 - u);
#pragma unroll
    for (int k = 0; k < (1 << R); k++) {
      if (k & half) continue;
      const u64x2 tp = tw_load(t.tw + (1 << u) + (k >> (R - u)));
      const u64 a = csub(x[k], m.two_q);
      const u64 v = mul_shoup_lazy(x[k | half], tp.x, tp.y, m.q);
      x[k] = a + v;
      x[k | half] = a + m.two_q - v;
    }
  }
  u64 *__restrict__ dst = dec + limb * (size_t)c.n + p;
#pragma unroll
  for (int k = 0; k < (1 << R); k++) dst[(size_t)k * G] = x[k];  // lazy [0, 4q): the block stages are guarded
}

// INV_D: the data limbs' sums go back to coefficients too (BFV); CKKS keeps them in NTT form.  SHOUP: `keys` = the key's Shoup
// quotients; sums of lazy products (< 2q each) stay below 2^64 for up to 16 digits of a 59-bit prime, wider primes fold after
// every term.
template <int LB, bool INV_D, bool SHOUP, bool GUARD>
__global__ __launch_bounds__((1 << LB) / 16, 3) void k_iks_special(DevCtx c, const u64 *__restrict__ dec, const u64 *__restrict__ key,
                                                                    const u64 *__restrict__ keys, u64 *__restrict__ prodD,
                                                                    u64 *__restrict__ prodS, int nl, int S0, unsigned cc) {
  __shared__ u64 lds[lds_words(LB)];
  // Every workgroup of a (key prime, block) pair reads the same 2 nl (x 2 with quotients) key blocks: ciphertext index fastest,
  // and -- consecutive workgroup ids go to consecutive XCDs -- the id is remapped so that one XCD's L2 sees the whole run
  // of ciphertexts of a pair (the grid is a multiple of 8: 2^S0 blocks per limb).
  const unsigned per_xcd = gridDim.x >> 3;
  const unsigned wid = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  const size_t ct = wid % cc;
  const unsigned pair = wid / cc;
  const int b = (int)(pair & ((1u << S0) - 1));
  const int I = (int)(pair >> S0);
  const int ki = (I == nl) ? c.K - 1 : I;
  const Mod m = c.mods[ki];
  const NttTable t = ntt_table(c, ki);
  const size_t N = (size_t)c.n, off = (size_t)b << LB;
  const bool fold = m.bits > 59;
  u64 acc0[16], acc1[16];
#pragma unroll
  for (int r = 0; r < 16; r++) acc0[r] = acc1[r] = 0;
#pragma nounroll
  for (int J = 0; J < nl; J++) {
    const u64 *__restrict__ in = dec + ((ct * nl + J) * (size_t)(nl + 1) + I) * N + off;
    const size_t kw = (((size_t)J * 2) * c.K + ki) * N + off, kw1 = kw + (size_t)c.K * N;
    ntt_fwd_block<LB, GUARD>(
        lds, [&](int, int i) { return in[i]; },
        [&](int r, int i, u64 v) {
          if (SHOUP) {
            acc0[r] += mul_shoup_lazy(v, key[kw + i], keys[kw + i], m.q);
            acc1[r] += mul_shoup_lazy(v, key[kw1 + i], keys[kw1 + i], m.q);
            if (fold) {
              acc0[r] = csub(acc0[r], m.two_q);
              acc1[r] = csub(acc1[r], m.two_q);
            }
          } else {
            const u64 x = canon_fwd<GUARD>(v, m);
            acc0[r] = add_mod(acc0[r], mul_mod(x, key[kw + i], m), m.q);
            acc1[r] = add_mod(acc1[r], mul_mod(x, key[kw1 + i], m), m.q);
          }
        },
        t, m, S0, b);
    block_sync_lds();  // the next transform's first pass rewrites words other wavefronts have just read
  }
  if (SHOUP) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      acc0[r] = reduce64(acc0[r], m);
      acc1[r] = reduce64(acc1[r], m);
    }
  }
  u64 *__restrict__ d0 = (I == nl ? prodS + (ct * 2 + 0) * N : prodD + ((ct * 2 + 0) * nl + I) * N) + off;
  u64 *__restrict__ d1 = (I == nl ? prodS + (ct * 2 + 1) * N : prodD + ((ct * 2 + 1) * nl + I) * N) + off;
  if (!INV_D && I != nl) {
    using P = PassIdx<LB, LB - 2, 2>;  // the forward transform's final register layout
    int hi[P::NG], lo[P::NG];
    P::groups((int)threadIdx.x, hi, lo);
#pragma unroll
    for (int g = 0; g < P::NG; g++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        d0[P::elem(hi[g], lo[g], k)] = acc0[g * 4 + k];
        d1[P::elem(hi[g], lo[g], k)] = acc1[g * 4 + k];
      }
    return;
  }
  ntt_inv_block<LB>(lds, [&](int r, int) { return acc0[r]; }, [&](int, int i, u64 v) { d0[i] = v; }, t, m, S0, b);
  block_sync_lds();
  ntt_inv_block<LB>(lds, [&](int r, int) { return acc1[r]; }, [&](int, int i, u64 v) { d1[i] = v; }, t, m, S0, b);
}

// BFV: everything behind k_iks_special in one kernel -- (ct, component, 256 positions): the strided last stages of the special
// limb's inverse transform, N^-1, + q_sp/2 -> t (2^R values in registers); then per data prime the same stages on its limb,
// N^-1, minus (t mod q_j + the rounding fix), times q_sp^-1, plus the addend -> coefficient form.  Replaces two strided passes
// (in place: a read and a write of 2 (nl + 1) limbs), k_divround_tmod (2 nl limbs written, read back) and k_divround_finish.
template <int R>
__global__ __launch_bounds__(256) void k_iks_finish(DevCtx c, const u64 *__restrict__ prodD, const u64 *__restrict__ prodS,
                                                    const u64 *addend, size_t addend_stride, int add_c1, u64 *out /* may be the addend */,
                                                    int nl, u32 ginv /* BFV rotation: gather the addend (then out is not the addend) */) {
  const int G = c.n >> R;
  const int per = G / 256;
  const size_t cc = blockIdx.x / per;  // ct * 2 + comp
  const int p = (blockIdx.x % per) * 256 + threadIdx.x;
  const size_t ct = cc >> 1;
  const int comp = (int)(cc & 1);
  const size_t N = (size_t)c.n;
  auto inverse_stages = [&](u64(&x)[1 << R], const Mod &m, const NttTable &t) {
#pragma unroll
    for (int u = R - 1; u >= 0; u--) {
      const int half = 1 << (R - 1 - u);
#pragma unroll
      for (int k = 0; k < (1 << R); k++) {
        if (k & half) continue;
        const u64x2 tp = tw_load(t.itw + (1 << u) + (k >> (R - u)));
        const u64 a = x[k], b2 = x[k | half];
        x[k] = csub(a + b2, m.two_q);
        x[k | half] = mul_shoup_lazy(a + m.two_q - b2, tp.x, tp.y, m.q);
      }
    }
  };
  u64 t[1 << R];
  {
    const Mod ms = c.mods[c.K - 1];
    const u64 *__restrict__ src = prodS + cc * N + p;
#pragma unroll
    for (int k = 0; k < (1 << R); k++) t[k] = src[(size_t)k * G];
    inverse_stages(t, ms, ntt_table(c, c.K - 1));
    const u64 half = ms.q >> 1;
#pragma unroll
    for (int k = 0; k < (1 << R); k++) t[k] = add_mod(scale_inv_n(t[k], ms), half, ms.q);
  }
  const u64 half = c.mods[c.K - 1].q >> 1;
  const bool add = addend && (comp == 0 || add_c1);
#pragma nounroll
  for (int j = 0; j < nl; j++) {
    const Mod m = c.mods[j];
    const u64 *__restrict__ src = prodD + (cc * nl + j) * N + p;
    u64 x[1 << R];
#pragma unroll
    for (int k = 0; k < (1 << R); k++) x[k] = src[(size_t)k * G];
    inverse_stages(x, m, ntt_table(c, j));
    const u64 fix = round_fix(half, m);
    const u64 inv = c.cst->inv_special[j], inv_s = c.cst->inv_special_s[j];
    u64 *o = out + (cc * nl + j) * N + p;
    const u64 *cin = add ? addend + ct * addend_stride + ((size_t)comp * nl + j) * N + p : nullptr;
#pragma unroll
    for (int k = 0; k < (1 << R); k++) {
      const u64 tm = add_mod(reduce64(t[k], m), fix, m.q);
      u64 v = mul_shoup(sub_mod(scale_inv_n(x[k], m), tm, m.q), inv, inv_s, m.q);
      if (add) {
        if (ginv) {  // workgroup-uniform
          bool neg;
          const u64 a = (cin - p)[galois_coef_src((u32)(k * G + p), ginv, c.logn, neg)];
          v = add_mod(v, neg ? neg_mod(a, m.q) : a, m.q);
        } else {
          v = add_mod(v, cin[(size_t)k * G], m.q);
        }
      }
      o[(size_t)k * G] = v;
    }
  }
}
static int iks_finish(abc_hip_ctx *c, const u64 *prodD, const u64 *prodS, const KsOperands &o) {
  const int S0 = c->logn - big_block_log();
  const int G = c->n >> S0;
  const dim3 grid((unsigned)(o.count * 2 * (G / 256)));
  hipLaunchKernelGGL((S0 == 3 ? k_iks_finish<3> : k_iks_finish<4>), grid, dim3(256), 0, c->stream, c->dc, prodD, prodS, o.addend, o.addend_stride,
                     o.add_c1, o.out, o.nl, o.gather);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// KsFront::iks (N = 2^15 / 2^16, 4096-point blocks).  On return prodS holds the special limb's sums half-way back to
// coefficients (strided stages left), prodD the data limbs' -- likewise for BFV, in NTT form for CKKS
static int iks_front(abc_hip_ctx *c, const u64 *tc, size_t tcs, const u64 *key, u64 *dec, u64 *prodD, u64 *prodS, int nl, size_t cc, u32 ginv,
                     bool guard) {
  const int S0 = c->logn - big_block_log();
  if (S0 != 3 && S0 != 4) { set_error("iks_front: N = 2^15 / 2^16 with 4096-point blocks only"); return 1; }
  const size_t limbs = cc * nl * (nl + 1);
  const int G = c->n >> S0;
  const dim3 g0((unsigned)(limbs * (G / 256)));
  if (S0 == 3) hipLaunchKernelGGL(k_iks_pass0<3>, g0, dim3(256), 0, c->stream, c->dc, tc, tcs, dec, nl, ginv);
  else hipLaunchKernelGGL(k_iks_pass0<4>, g0, dim3(256), 0, c->stream, c->dc, tc, tcs, dec, nl, ginv);
  ABC_HIP_CHECK(hipGetLastError());
  const dim3 g1((unsigned)((cc * (nl + 1)) << S0));
  const u64 *keys = key_shoup(c, key);
  const bool ckks = c->scheme == 2;
  // unguarded butterflies (!guard) where every key prime leaves the room: [0, 4q) out of the strided pass, + 4q per block stage = 52q < 2^64
#define ABC_IKS(INV_D, SHOUP)                                                                                                        \
  do {                                                                                                                               \
    if (guard)                                                                                                                       \
      hipLaunchKernelGGL((k_iks_special<12, INV_D, SHOUP, true>), g1, dim3(256), 0, c->stream, c->dc, dec, key, keys, prodD, prodS, \
                         nl, S0, (unsigned)cc);                                                                                      \
    else                                                                                                                             \
      hipLaunchKernelGGL((k_iks_special<12, INV_D, SHOUP, false>), g1, dim3(256), 0, c->stream, c->dc, dec, key, keys, prodD, prodS, \
                         nl, S0, (unsigned)cc);                                                                                      \
  } while (0)
  if (keys) { if (ckks) ABC_IKS(false, true); else ABC_IKS(true, true); }
  else { if (ckks) ABC_IKS(false, false); else ABC_IKS(true, false); }
#undef ABC_IKS
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// o.gather: BFV with front == iks only (seq_folds_permutation)
int keyswitch_generic(abc_hip_ctx *c, KsFront front, const KsOperands &all) {
  const size_t count = all.count, N = (size_t)c->n;
  const int nl = all.nl;
  const u64 *key = all.key;
  if (!count) return 0;
  const bool ckks = (c->scheme == 2);
  // workspace per ciphertext (words): tcoef nl + dec nl(nl+1) + prodD 2nl + prodS 2 + tmod 2nl
  const size_t per_ct = ((size_t)nl + (size_t)nl * (nl + 1) + 2 * nl + 2 + 2 * nl) * N;
  const size_t chunk = even_chunks((size_t)(c->logn > 14 ? 4 : 1) << 30, per_ct, count);  // <= 1 GiB of scratch per chunk (big rings: 4 GiB)
  if (ensure_workspace(c, chunk * per_ct * 8)) return 1;
  u64 *tcoef = (u64 *)c->ws;
  u64 *dec = tcoef + chunk * nl * N;
  u64 *prodD = dec + chunk * nl * (nl + 1) * N;
  u64 *prodS = prodD + chunk * 2 * nl * N;
  u64 *tmod = prodS + chunk * 2 * N;
  const LimbMap dmap = key_limb_map(c, nl);
  LimbMap smap{};
  smap.id[0] = c->K - 1;
  for (size_t off = 0; off < count; off += chunk) {
    const size_t cc = (count - off < chunk) ? count - off : chunk;
    const KsOperands o = all.slice(off, cc, N);
    const u64 *tc = o.target;
    size_t tcs = o.target_stride;
    if (ckks) {  // CKKS targets are in NTT form: back to coefficients first
      ABC_HIP_CHECK(hipMemcpy2DAsync(tcoef, nl * N * 8, o.target, o.target_stride * 8, nl * N * 8, cc, hipMemcpyDeviceToDevice,
                                     c->stream));
      if (launch_ntt_inv(c, tcoef, dmap, nl, cc * nl)) return 1;
      tc = tcoef;
      tcs = nl * N;
    }
    if (front == KsFront::fp && launch_ks_expand_ntt_fp(c, tc, tcs, dec, dmap, nl, cc)) return 1;
    const bool iks = front == KsFront::iks;
    if (iks && iks_front(c, tc, tcs, key, dec, prodD, prodS, nl, cc, o.gather, c->facts.guard)) return 1;
    if (iks && !ckks) {  // inner products done, block stages of the inverse transforms too: one kernel does the rest
      if (iks_finish(c, prodD, prodS, o)) return 1;
      continue;
    }
    if (iks) {  // CKKS: the special limb's strided stages (integers, like its block stages: k_iks_special), then as ever
      if (launch_ntt_inv_strided_part(c, prodS, smap, 1, cc * 2, true)) return 1;
      if (launch_ks_tmod(c, prodS, tmod, nl, cc * 2)) return 1;
      if (launch_ntt_fwd(c, tmod, dmap, nl, cc * 2 * nl)) return 1;
    } else {
      if (front == KsFront::plain) {
        hipLaunchKernelGGL(k_ks_expand, dim3(grid_for(cc * nl * N, 256)), dim3(256), 0, c->stream, c->dc, tc, tcs, dec, nl, cc);
        ABC_HIP_CHECK(hipGetLastError());
        if (launch_ntt_fwd(c, dec, dmap, nl + 1, cc * nl * (nl + 1))) return 1;
      }
      hipLaunchKernelGGL(k_ks_inner, dim3(grid_for(cc * (nl + 1) * N, 256)), dim3(256), 0, c->stream, c->dc, dec, key, prodD,
                         prodS, nl, cc);
      ABC_HIP_CHECK(hipGetLastError());
      if (launch_ntt_inv(c, prodS, smap, 1, cc * 2)) return 1;
      if (launch_ks_tmod(c, prodS, tmod, nl, cc * 2)) return 1;
      if (ckks) {
        if (launch_ntt_fwd(c, tmod, dmap, nl, cc * 2 * nl)) return 1;
      } else {
        if (launch_ntt_inv(c, prodD, dmap, nl, cc * 2 * nl)) return 1;
      }
    }
    if (launch_ks_finish(c, prodD, tmod, o.out, o.addend, o.addend_stride, o.add_c1, nl, cc)) return 1;
  }
  return 0;
}

// ---- Galois automorphism x -> x^elt on [polys][nl][N] ----
__global__ __launch_bounds__(256) void k_galois(DevCtx c, const u64 *in, u64 *out, int nl, size_t polys, u32 elt, int ntt_form) {
  const size_t items = polys * nl * (size_t)c.n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t limb = it >> c.logn;
    const u32 i = (u32)(it & (c.n - 1));
    const u64 *src = in + limb * c.n;
    u64 *dst = out + limb * c.n;
    if (ntt_form) {
      // slot i holds the evaluation at psi^(2*bitrev(i)+1); gather from the slot holding exponent*elt
      const u32 rev = bitrev32(i + (u32)c.n, c.logn + 1);
      const u64 idx = (((u64)elt * rev) >> 1) & (u64)(c.n - 1);
      dst[i] = src[bitrev32((u32)idx, c.logn)];
    } else {
      const u64 raw = (u64)i * elt;
      const u32 idx = (u32)(raw & (u64)(c.n - 1));
      u64 v = src[i];
      if ((raw >> c.logn) & 1) v = neg_mod(v, c.mods[limb % nl].q);
      dst[idx] = v;
    }
  }
}

int launch_galois(abc_hip_ctx *c, const u64 *in, u64 *out, int nl, size_t polys, uint32_t elt, bool ntt_form) {
  const size_t items = polys * nl * (size_t)c->n;
  if (!items) return 0;
  hipLaunchKernelGGL(k_galois, dim3(grid_for(items, 256)), dim3(256), 0, c->stream, c->dc, in, out, nl, polys, elt,
                     ntt_form ? 1 : 0);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- CKKS rescale: drop limb nl-1 with rounding (divide_and_round_q_last_ntt) ----
__global__ __launch_bounds__(256) void k_gather_last(DevCtx c, const u64 *in, u64 *last, int nl, size_t polys) {
  const size_t items = polys * c.n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t p = it >> c.logn, k = it & (c.n - 1);
    last[it] = in[(p * nl + (nl - 1)) * c.n + k];
  }
}

// ---- the same for rings that fit LDS: two kernels instead of five (steps A and B of abc_ntt.hpp's "divide and round") ----
// R1 (poly): inverse transform of the last limb, read in place, + q_last/2 -> scratch.
// R2 (poly, j < nl-1): scratch + rounding fix as operand of a forward transform modulo q_j in LDS, then
//     (in_j - transform) * q_last^-1 -> out_j.  The nl-1 workgroups that read one scratch polynomial share an L2 (xcd_slot).
//     7 + 2 limb transfers per polynomial instead of 23.
// !MIXED: every prime below 2^50, fp64 throughout (no reduction of the operand: the fp64 bound absorbs a 50-bit one).
// MIXED (chains that contain a prime above 2^50): the arithmetic chosen per prime -- the inverse transform runs in that of the
// dropped prime (fp_last), each forward transform in that of its own prime j (bit j of fpmask: below 2^50), workgroup-uniform.
// R1 keeps its all-fp64 form as a kernel of its own: as an instantiation of the mixed one its register count changed.
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_rescale_intt_fp(DevCtx c, const u64 *__restrict__ in, u64 *__restrict__ last,
                                                                    int nl) {
  __shared__ double lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB;
  const Mod m = mod_at(c, nl - 1);
  const FpTable t = fp_table(c, nl - 1);
  const double half = (double)(m.q >> 1);
  const u64 *__restrict__ src = in + ((size_t)blockIdx.x * nl + (nl - 1)) * N;
  u64 *__restrict__ dst = last + (size_t)blockIdx.x * N;
  ntt_inv_block_a<LB, FpArith>(
      lds, [&](int, int i) { return fp_from_u64(src[i]); },
      [&](int, int i, double v) { dst[i] = fp_to_canon(fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd) + half, m.qd, m.qinv); }, t, m, 0,
      0);
}
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_rescale_intt_mixed(DevCtx c, const u64 *__restrict__ in, u64 *__restrict__ last, int nl,
                                                                       int fp_last) {
  __shared__ u64 lds_raw[lds_words(LB)];
  const size_t N = (size_t)1 << LB;
  const u64 *__restrict__ src = in + ((size_t)blockIdx.x * nl + (nl - 1)) * N;
  u64 *__restrict__ dst = last + (size_t)blockIdx.x * N;
  if (fp_last)
    divround_to_coef<LB, FpArith>(reinterpret_cast<double *>(lds_raw), mod_at(c, nl - 1), fp_table(c, nl - 1), src, dst);
  else
    divround_to_coef<LB, IntArith<true>>(lds_raw, c.mods[nl - 1], ntt_table(c, nl - 1), src, dst);
}
template <int LB, bool MIXED>
__global__ __launch_bounds__((1 << LB) / 16) void k_rescale_ntt(DevCtx c, const u64 *__restrict__ in, const u64 *__restrict__ last,
                                                                u64 *__restrict__ out, int nl, int npoly, u32 fpmask) {
  __shared__ u64 lds_raw[lds_words(LB)];
  int j;
  size_t p;
  xcd_slot(blockIdx.x, nl - 1, npoly, j, p);
  const size_t N = (size_t)1 << LB;
  const Mod m = MIXED ? c.mods[j] : mod_at(c, j);
  // MIXED: the dropped prime may be wider than 2^52 -- the rounding fix stays an integer and the fp64 load reduces first (REDUCE)
  const auto fix = round_fix<std::conditional_t<MIXED, u64, double>>(c.mods[nl - 1].q >> 1, m);
  const DropInv d = inv_qlast_at(c, nl - 1, j);
  const u64 *__restrict__ src = last + p * N;
  const u64 *__restrict__ x = in + (p * nl + j) * N;
  u64 *__restrict__ o = out + (p * (nl - 1) + j) * N;
  if constexpr (!MIXED)
    divround_finish<LB, FpArith, false, false>(reinterpret_cast<double *>(lds_raw), m, fp_table(c, j), fix, d, src, x, nullptr, o);
  else if ((fpmask >> j) & 1u)
    divround_finish<LB, FpArith, true, false>(reinterpret_cast<double *>(lds_raw), mod_at(c, j), fp_table(c, j), fix, d, src, x, nullptr, o);
  else
    divround_finish<LB, IntArith<true>, false, false>(lds_raw, m, ntt_table(c, j), fix, d, src, x, nullptr, o);
}
template <int LB, bool MIXED>
static int launch_rescale_lds(abc_hip_ctx *c, const u64 *in, u64 *out, int nl, size_t polys, u32 fpmask) {
  const size_t N = (size_t)1 << LB;
  if (ensure_workspace(c, polys * N * 8)) return 1;
  u64 *last = (u64 *)c->ws;
  const dim3 block((1 << LB) / 16);
  if constexpr (MIXED)
    hipLaunchKernelGGL(k_rescale_intt_mixed<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, in, last, nl, (int)((fpmask >> (nl - 1)) & 1u));
  else
    hipLaunchKernelGGL(k_rescale_intt_fp<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, in, last, nl);
  hipLaunchKernelGGL((k_rescale_ntt<LB, MIXED>), dim3((unsigned)(polys * (nl - 1))), block, 0, c->stream, c->dc, in, last, out, nl,
                     (int)polys, fpmask);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_rescale(abc_hip_ctx *c, const u64 *in, u64 *out, int size, int nl, size_t count) {
  if (nl < 2) { set_error("rescale: no limb left to drop"); return 1; }
  const size_t N = (size_t)c->n, polys = count * size;
  if (!polys) return 0;
  const RescaleRoute r = route_rescale(c->facts, nl, in == out);
  if (r.kind == Rescale::mixed)  // a prime above 2^50 in the chain
    return dispatch_logn<10, 14>(c->logn, [&](auto LB) { return launch_rescale_lds<decltype(LB)::value, true>(c, in, out, nl, polys, r.fpmask); });
  if (r.kind == Rescale::fp)
    return dispatch_logn<10, 14>(c->logn, [&](auto LB) { return launch_rescale_lds<decltype(LB)::value, false>(c, in, out, nl, polys, 0u); });
  if (ensure_workspace(c, (polys * N + polys * (nl - 1) * N) * 8)) return 1;
  u64 *last = (u64 *)c->ws, *tmod = last + polys * N;
  hipLaunchKernelGGL(k_gather_last, dim3(grid_for(polys * N, 256)), dim3(256), 0, c->stream, c->dc, in, last, nl, polys);
  ABC_HIP_CHECK(hipGetLastError());
  LimbMap lmap{};
  lmap.id[0] = nl - 1;
  if (launch_ntt_inv(c, last, lmap, 1, polys)) return 1;
  if (launch_divround_tmod(c, last, tmod, nl - 1, nl - 1, polys)) return 1;
  if (launch_ntt_fwd(c, tmod, key_limb_map(c, nl - 1), nl - 1, polys * (nl - 1))) return 1;
  return launch_divround_finish(c, in, nl, tmod, out, c->dc.cst->inv_qlast[nl - 1], c->dc.cst->inv_qlast_s[nl - 1], nullptr, 0, false, nl - 1,
                                polys);
}

// ---- multiply_plain + rescale in one: the product with the plaintext formed in the loads of R1 and R2 (the policies' mul_u64) ----
// Kernels of their own beside the unfused ones, whose device code stays what it was.  Polynomial p belongs to ciphertext p / size, whose
// plaintext row starts at (p / size) * plain_stride ([nl][N], stride 0: one row for the batch).  R2's nl - 1 workgroups of a polynomial
// share an L2 as before (xcd_slot); with one row for the batch, limb j of the plaintext is shared by every workgroup of that limb.
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_mulplain_rescale_intt_fp(DevCtx c, const u64 *__restrict__ in, const u64 *__restrict__ plain,
                                                                             size_t plain_stride, u64 *__restrict__ last, int size, int nl) {
  __shared__ double lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB, p = blockIdx.x;
  divround_to_coef<LB, FpArith, true>(lds, mod_at(c, nl - 1), fp_table(c, nl - 1), in + (p * nl + (nl - 1)) * N, last + p * N,
                                      plain + (p / size) * plain_stride + (size_t)(nl - 1) * N);
}
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_mulplain_rescale_intt_mixed(DevCtx c, const u64 *__restrict__ in, const u64 *__restrict__ plain,
                                                                                size_t plain_stride, u64 *__restrict__ last, int size, int nl,
                                                                                int fp_last) {
  __shared__ u64 lds_raw[lds_words(LB)];
  const size_t N = (size_t)1 << LB, p = blockIdx.x;
  const u64 *__restrict__ src = in + (p * nl + (nl - 1)) * N;
  const u64 *__restrict__ pl = plain + (p / size) * plain_stride + (size_t)(nl - 1) * N;
  u64 *__restrict__ dst = last + p * N;
  if (fp_last)
    divround_to_coef<LB, FpArith, true>(reinterpret_cast<double *>(lds_raw), mod_at(c, nl - 1), fp_table(c, nl - 1), src, dst, pl);
  else
    divround_to_coef<LB, IntArith<true>, true>(lds_raw, c.mods[nl - 1], ntt_table(c, nl - 1), src, dst, pl);
}
template <int LB, bool MIXED>
__global__ __launch_bounds__((1 << LB) / 16) void k_mulplain_rescale_ntt(DevCtx c, const u64 *__restrict__ in, const u64 *__restrict__ plain,
                                                                         size_t plain_stride, const u64 *__restrict__ last, u64 *__restrict__ out,
                                                                         int size, int nl, int npoly, u32 fpmask) {
  __shared__ u64 lds_raw[lds_words(LB)];
  int j;
  size_t p;
  xcd_slot(blockIdx.x, nl - 1, npoly, j, p);
  const size_t N = (size_t)1 << LB;
  const Mod m = MIXED ? c.mods[j] : mod_at(c, j);
  const auto fix = round_fix<std::conditional_t<MIXED, u64, double>>(c.mods[nl - 1].q >> 1, m);
  const DropInv d = inv_qlast_at(c, nl - 1, j);
  const u64 *__restrict__ src = last + p * N;
  const u64 *__restrict__ x = in + (p * nl + j) * N;
  const u64 *__restrict__ pl = plain + (p / size) * plain_stride + (size_t)j * N;
  u64 *__restrict__ o = out + (p * (nl - 1) + j) * N;
  if constexpr (!MIXED)
    divround_finish<LB, FpArith, false, false, true>(reinterpret_cast<double *>(lds_raw), m, fp_table(c, j), fix, d, src, x, nullptr, o, pl);
  else if ((fpmask >> j) & 1u)
    divround_finish<LB, FpArith, true, false, true>(reinterpret_cast<double *>(lds_raw), mod_at(c, j), fp_table(c, j), fix, d, src, x, nullptr, o, pl);
  else
    divround_finish<LB, IntArith<true>, false, false, true>(lds_raw, m, ntt_table(c, j), fix, d, src, x, nullptr, o, pl);
}
template <int LB, bool MIXED>
static int launch_mulplain_rescale_lds(abc_hip_ctx *c, const u64 *in, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl,
                                       size_t polys, u32 fpmask) {
  const size_t N = (size_t)1 << LB;
  if (ensure_workspace(c, polys * N * 8)) return 1;
  u64 *last = (u64 *)c->ws;
  const dim3 block((1 << LB) / 16);
  if constexpr (MIXED)
    hipLaunchKernelGGL(k_mulplain_rescale_intt_mixed<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, in, plain, plain_stride, last, size, nl,
                       (int)((fpmask >> (nl - 1)) & 1u));
  else
    hipLaunchKernelGGL(k_mulplain_rescale_intt_fp<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, in, plain, plain_stride, last, size, nl);
  hipLaunchKernelGGL((k_mulplain_rescale_ntt<LB, MIXED>), dim3((unsigned)(polys * (nl - 1))), block, 0, c->stream, c->dc, in, plain, plain_stride,
                     last, out, size, nl, (int)polys, fpmask);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// out [count][size][nl-1][N] = rescale(ct (.) plain): fused into the LDS-resident rescale, or the product into arena 1 (the products'
// arena: abc_context.hpp) and launch_rescale on it.  The caller has checked the scheme, the stride and the overlaps.
int launch_mulplain_rescale(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl, size_t count) {
  if (nl < 2) { set_error("multiply_plain_rescale: no limb left to drop"); return 1; }
  const size_t polys = count * size;
  if (!polys) return 0;
  const MulPlainRescaleRoute r = route_mulplain_rescale(c->facts, nl);
  if (r.fused && r.rescale.kind == Rescale::mixed)
    return dispatch_logn<10, 14>(c->logn, [&](auto LB) {
      return launch_mulplain_rescale_lds<decltype(LB)::value, true>(c, ct, plain, plain_stride, out, size, nl, polys, r.rescale.fpmask);
    });
  if (r.fused)
    return dispatch_logn<10, 14>(c->logn, [&](auto LB) {
      return launch_mulplain_rescale_lds<decltype(LB)::value, false>(c, ct, plain, plain_stride, out, size, nl, polys, 0u);
    });
  if (ensure_aux(c, 1, polys * nl * (size_t)c->n * 8)) return 1;
  u64 *prod = (u64 *)c->aux[1];
  if (ckks_multiply_plain(c, ct, plain, plain_stride, prod, size, nl, count)) return 1;
  return launch_rescale(c, prod, out, size, nl, count);
}

int launch_drop_last(abc_hip_ctx *c, const u64 *in, u64 *out, int size, int nl, size_t count) {
  if (nl < 2) { set_error("mod_switch: no limb left to drop"); return 1; }
  const size_t N = (size_t)c->n, polys = count * size;
  if (!polys) return 0;
  ABC_HIP_CHECK(hipMemcpy2DAsync(out, (nl - 1) * N * 8, in, nl * N * 8, (nl - 1) * N * 8, polys, hipMemcpyDeviceToDevice,
                                 c->stream));
  return 0;
}

// ---- the pieces of multiply_const_sum's composed route (ABC_HIP_NO_CONST_MAC_SUM; the K-term kernel is further down) ----
// the constant plaintext: plain [nl][N], every word of limb j = w[j] (by value)
struct ConstWords {
  u64 w[kMaxLimbs];
};
__global__ __launch_bounds__(256) void k_const_plain_fill(DevCtx c, ConstWords cw, u64 *plain) {
  const u32 spans = (u32)c.n / kTensorSumSpan;  // one workgroup per span of one limb: the word is workgroup-uniform
  const u64 v = cw.w[blockIdx.x / spans];
  *reinterpret_cast<u64x2 *>(plain + (size_t)blockIdx.x * kTensorSumSpan + 2 * threadIdx.x) = u64x2{v, v};
}
int launch_const_plain_fill(abc_hip_ctx *c, const u64 *w, u64 *plain, int nl) {
  ConstWords cw{};
  for (int j = 0; j < nl; j++) cw.w[j] = w[j];
  hipLaunchKernelGGL(k_const_plain_fill, dim3((unsigned)(nl * (c->n / kTensorSumSpan))), dim3(256), 0, c->stream, c->dc, cw, plain);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
// in [polys][from_nl][N] -> out [polys][nl][N], the first nl limbs of each: launch_drop_last repeated from_nl - nl times, in one copy
int launch_drop_to(abc_hip_ctx *c, const u64 *in, u64 *out, int from_nl, int nl, size_t polys) {
  const size_t N = (size_t)c->n;
  if (!polys) return 0;
  ABC_HIP_CHECK(hipMemcpy2DAsync(out, nl * N * 8, in, from_nl * N * 8, nl * N * 8, polys, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// ---- CKKS plaintext ops (NTT-form plaintext [nl][N]) ----
__global__ __launch_bounds__(256) void k_ckks_plain(DevCtx c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out,
                                                    int size, int nl, size_t count, int op) {
  const size_t pw = (size_t)nl * c.n;
  const size_t items = count * size * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ctp = it / pw, w = it % pw;
    const size_t ci = ctp / size;
    const int p = (int)(ctp % size);
    const Mod m = c.mods[w >> c.logn];
    const u64 pv = plain[ci * plain_stride + w];
    u64 v = ct[it];
    if (op == 0) v = mul_mod(v, pv, m);
    else if (p == 0) v = (op == 1) ? add_mod(v, pv, m.q) : sub_mod(v, pv, m.q);
    out[it] = v;
  }
}
int ckks_multiply_plain(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl,
                        size_t count) {
  const size_t items = count * size * nl * (size_t)c->n;
  if (!items) return 0;
  hipLaunchKernelGGL(k_ckks_plain, dim3(grid_for(items, 256)), dim3(256), 0, c->stream, c->dc, ct, plain, plain_stride, out, size,
                     nl, count, 0);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
int ckks_add_plain(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl, size_t count,
                   int sub) {
  const size_t items = count * size * nl * (size_t)c->n;
  if (!items) return 0;
  hipLaunchKernelGGL(k_ckks_plain, dim3(grid_for(items, 256)), dim3(256), 0, c->stream, c->dc, ct, plain, plain_stride, out, size,
                     nl, count, sub ? 2 : 1);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- CKKS plaintext multiply-accumulate sum: out = (carry or 0) + sum over the launch's terms of plain_k (.) ct_k ----
// The plaintext twin of k_ckks_tensor_sum, for abc_hip_multiply_plain_sum and the inner sums of abc_hip_diag_matvec_bsgs.  One
// workgroup owns kTensorSumSpan consecutive coefficients of ONE limb of one ciphertext and all SIZE components of it: the modulus is
// workgroup-uniform, a term's plaintext words are loaded once for the 2 or 3 components, every lane moves 16 bytes per load and
// store, and a term's 1 + SIZE loads are issued before the previous term's arithmetic.  The term pointers travel by value and the
// loop over them is unrolled (the record is indexed by constants only).  The carried value is a POINTER: the addend on a call's
// first launch, `out` on the later ones, null where there is neither.  A lane reads its own words of it before it writes them to
// `out`, so out == carry needs no copy.  Results are exact modular sums in canonical form, whatever the order: bit-identical to
// k_ckks_plain per term and k_addsub.
struct PlainMacTerms {
  const u64 *ct[kPlainMacTerms], *plain[kPlainMacTerms];
};
// Integer limbs: the 128-bit products accumulate lazily and are reduced once per launch.  A launch sums at most kPlainMacTerms
// products, each at most (q - 1)^2, and the carried word (below q: less than one product): (T + 1) (q - 1)^2 < 2^128 must hold for
// the widest prime a context accepts, 2^60 -- 2^(128 - 2 * 60) = 256, so T could be 255; the launch boundary is the reduction.
static_assert(kPlainMacTerms + 1 <= (1 << (128 - 2 * kTensorSumPrimeBits)), "plain mac sum: the 128-bit accumulator would overflow within one launch");
// fp64 limbs (q < 2^50): the carried word is below q, every product is |.| < q (fp_mulmod), and integer-valued doubles are exact up
// to 2^53 >= 8 q.  So at most 7 products may follow the carried word -- or a re-centred accumulator, |.| <= q/2 -- before the next
// re-centring.  The accumulators are re-centred after every kPlainMacFpTerms = 4 terms of a launch (carried + 4 products < 5 q,
// then q/2 + 4 products < 4.5 q); a launch of 8 terms cannot do without one (1 + 8 > 8).  fp_to_canon centres the last group.
constexpr int kPlainMacFpTerms = 4;
static_assert(kPlainMacFpTerms + 1 <= 8, "plain mac sum: the fp64 accumulator would pass 2^53 between two re-centrings");

template <int SIZE>
struct PlainMacLoad {
  u64x2 p, c[SIZE];
};
template <int SIZE>
__device__ __forceinline__ PlainMacLoad<SIZE> plain_mac_load(const u64 *ct, const u64 *plain, size_t ct_off, size_t plain_off, size_t pw) {
  PlainMacLoad<SIZE> t;
  t.p = *reinterpret_cast<const u64x2 *>(plain + plain_off);
#pragma unroll
  for (int s = 0; s < SIZE; s++) t.c[s] = *reinterpret_cast<const u64x2 *>(ct + ct_off + s * pw);
  return t;
}

// one tile on the integers; pc: this lane's words of the carried value, or null
template <int SIZE>
__device__ __forceinline__ void plain_mac_int(const PlainMacTerms &t, int nt, const Mod &m, size_t ct_off, size_t plain_off, size_t pw,
                                              const u64 *pc, u64 *po) {
  U128 ax[SIZE], ay[SIZE];
#pragma unroll
  for (int s = 0; s < SIZE; s++) ax[s] = U128{0, 0}, ay[s] = U128{0, 0};
  if (pc) {  // workgroup-uniform
#pragma unroll
    for (int s = 0; s < SIZE; s++) {
      const u64x2 r = *reinterpret_cast<const u64x2 *>(pc + s * pw);
      ax[s].lo = r.x, ay[s].lo = r.y;
    }
  }
  PlainMacLoad<SIZE> cur = plain_mac_load<SIZE>(t.ct[0], t.plain[0], ct_off, plain_off, pw), nxt = cur;
#pragma unroll
  for (int k = 0; k < kPlainMacTerms; k++) {
    if (k < nt) {  // workgroup-uniform
      if (k + 1 < kPlainMacTerms && k + 1 < nt) nxt = plain_mac_load<SIZE>(t.ct[k + 1], t.plain[k + 1], ct_off, plain_off, pw);
#pragma unroll
      for (int s = 0; s < SIZE; s++) mac128(ax[s], cur.c[s].x, cur.p.x), mac128(ay[s], cur.c[s].y, cur.p.y);
      cur = nxt;
    }
  }
  const u64 r64 = reduce64(0ull - m.q, m);  // 2^64 mod q
#pragma unroll
  for (int s = 0; s < SIZE; s++) *reinterpret_cast<u64x2 *>(po + s * pw) = u64x2{reduce128(ax[s], r64, m), reduce128(ay[s], r64, m)};
}

// one tile in fp64 (q < 2^50)
template <int SIZE>
__device__ __forceinline__ void plain_mac_fp(const PlainMacTerms &t, int nt, const Mod &m, size_t ct_off, size_t plain_off, size_t pw,
                                             const u64 *pc, u64 *po) {
  const double q = m.qd, qinv = m.qinv;
  double ax[SIZE], ay[SIZE];
#pragma unroll
  for (int s = 0; s < SIZE; s++) ax[s] = 0, ay[s] = 0;
  if (pc) {  // workgroup-uniform
#pragma unroll
    for (int s = 0; s < SIZE; s++) {
      const u64x2 r = *reinterpret_cast<const u64x2 *>(pc + s * pw);
      ax[s] = fp_from_u64(r.x), ay[s] = fp_from_u64(r.y);
    }
  }
  PlainMacLoad<SIZE> cur = plain_mac_load<SIZE>(t.ct[0], t.plain[0], ct_off, plain_off, pw), nxt = cur;
#pragma unroll
  for (int k = 0; k < kPlainMacTerms; k++) {
    if (k < nt) {  // workgroup-uniform
      if (k + 1 < kPlainMacTerms && k + 1 < nt) nxt = plain_mac_load<SIZE>(t.ct[k + 1], t.plain[k + 1], ct_off, plain_off, pw);
      const double px = fp_from_u64(cur.p.x), py = fp_from_u64(cur.p.y);
#pragma unroll
      for (int s = 0; s < SIZE; s++) {
        ax[s] += fp_mulmod(fp_from_u64(cur.c[s].x), px, q, qinv);
        ay[s] += fp_mulmod(fp_from_u64(cur.c[s].y), py, q, qinv);
      }
      // carried value + kPlainMacFpTerms products < 5 q < 2^53 up to here (see kPlainMacFpTerms)
      if ((k + 1) % kPlainMacFpTerms == 0 && k + 1 < kPlainMacTerms) {
#pragma unroll
        for (int s = 0; s < SIZE; s++) ax[s] = fp_centre(ax[s], q, qinv), ay[s] = fp_centre(ay[s], q, qinv);
      }
      cur = nxt;
    }
  }
#pragma unroll
  for (int s = 0; s < SIZE; s++) *reinterpret_cast<u64x2 *>(po + s * pw) = u64x2{fp_to_canon(ax[s], q, qinv), fp_to_canon(ay[s], q, qinv)};
}

// tiles = count * nl * (N / kTensorSumSpan), tile -> (ciphertext, limb, span) with scalar arithmetic; fpmask, HAS_FP / HAS_INT as in
// k_ckks_tensor_sum.  carry: [count][SIZE][nl][N] like out (and possibly out itself), or null
template <bool HAS_FP, bool HAS_INT, int SIZE>
__global__ __launch_bounds__(256) void k_ckks_plain_mac_sum(DevCtx c, PlainMacTerms t, int nt, size_t plain_stride, const u64 *carry, u64 *out,
                                                            int nl, size_t tiles, u32 fpmask) {
  const u32 spans = (u32)c.n / kTensorSumSpan;
  const size_t pw = (size_t)nl * c.n;
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t limb = tile / spans;  // ct * nl + j
    const u32 span = (u32)(tile - limb * spans);
    const size_t ct = limb / (u32)nl;
    const int j = (int)(limb - ct * (u32)nl);
    const size_t w = (size_t)j * c.n + (size_t)span * kTensorSumSpan + 2 * threadIdx.x;  // word inside a polynomial
    const Mod m = mod_at(c, j);
    const size_t ct_off = ct * SIZE * pw + w, plain_off = ct * plain_stride + w;
    const u64 *pc = carry ? carry + ct_off : nullptr;
    if (HAS_FP && (!HAS_INT || ((fpmask >> j) & 1u))) plain_mac_fp<SIZE>(t, nt, m, ct_off, plain_off, pw, pc, out + ct_off);
    else plain_mac_int<SIZE>(t, nt, m, ct_off, plain_off, pw, pc, out + ct_off);
  }
}

// out [count][size][nl][N] = (addend or 0) + sum over k < n_terms of plain[k] (.) ct[k]; ct, plain: HOST arrays of device pointers;
// n_terms >= 1 (the caller copies the addend, or writes the zeros, of an empty sum), size 2 or 3, on stream c->stream
int launch_ckks_plain_mac_sum(abc_hip_ctx *c, const u64 *const *ct, const u64 *const *plain, size_t plain_stride, int n_terms, const u64 *addend,
                              u64 *out, int size, int nl, size_t count) {
  const size_t tiles = count * nl * ((size_t)c->n / kTensorSumSpan);
  if (!tiles || n_terms < 1) return 0;
  const u32 full = (1u << nl) - 1u;
  const u32 fpmask = (c->use_fp && (c->facts.data_fp(nl) || !c->sw.no_mixed)) ? c->facts.fp_data_mask(nl) : 0u;
  const size_t cap = 256 * 8 * 16;  // workgroups: every CU several times over, the tile loop beyond
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
  for (int k0 = 0; k0 < n_terms; k0 += kPlainMacTerms) {
    const int nt = n_terms - k0 < kPlainMacTerms ? n_terms - k0 : kPlainMacTerms;
    PlainMacTerms t;
    for (int k = 0; k < kPlainMacTerms; k++) t.ct[k] = ct[k0 + (k < nt ? k : 0)], t.plain[k] = plain[k0 + (k < nt ? k : 0)];
    const u64 *carry = k0 ? out : addend;
    auto go = [&](auto has_fp, auto has_int, auto sz) {
      hipLaunchKernelGGL((k_ckks_plain_mac_sum<decltype(has_fp)::value, decltype(has_int)::value, decltype(sz)::value>), grid, dim3(256), 0,
                         c->stream, c->dc, t, nt, plain_stride, carry, out, nl, tiles, fpmask);
    };
    auto by_size = [&](auto has_fp, auto has_int) {
      if (size == 3) go(has_fp, has_int, std::integral_constant<int, 3>{});
      else go(has_fp, has_int, std::integral_constant<int, 2>{});
    };
    if (fpmask == full) by_size(std::true_type{}, std::false_type{});
    else if (!fpmask) by_size(std::false_type{}, std::true_type{});
    else by_size(std::true_type{}, std::true_type{});
    ABC_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// ---- CKKS scalar-weighted sum: out = (carry or 0) + const (component 0) + sum over the launch's terms of w_k * ct_k ----
// k_ckks_plain_mac_sum with the plaintext of every term a CONSTANT: in NTT form the constant c is the polynomial whose every word of
// limb j is c mod q_j, so a term needs no plaintext load at all -- its weight is one word per limb, and the limb is workgroup-uniform.
// The weights and the additive constant travel BY VALUE in the kernel arguments (kConstMacTerms x kMaxLimbs words and kMaxLimbs
// more) and are indexed by the limb, which is workgroup-uniform: scalar loads from the kernel-argument segment, no private copy (the
// resource table shows no scratch), no device-side table, and the call stays capturable with the weights in its record.  Every term has its own polynomial
// stride: term k is laid out [count][SIZE][limbs[k]][N] with limbs[k] >= nl and its first nl limbs are read in place, which is
// abc_hip_mod_switch down to nl without the copy.  Tiles, the 16-byte accesses, the next term's loads ahead of the arithmetic, the
// carry by pointer (out == carry needs no copy) as in k_ckks_plain_mac_sum.  Results are exact modular sums in canonical form:
// bit-identical to k_ckks_plain per term on the constant plaintext, k_addsub, and k_ckks_plain's add on component 0.
struct ConstMacTerms {
  const u64 *ct[kConstMacTerms];
  u32 limbs[kConstMacTerms];           // polynomial stride of term k in limbs
  u64 w[kConstMacTerms][kMaxLimbs];    // weight of term k modulo q_j, canonical
  u64 cst[kMaxLimbs];                  // the additive constant modulo q_j (zeros where there is none, and on every launch after the first)
};
// The bounds of k_ckks_plain_mac_sum carry over: a weight is below q exactly as a plaintext word is.  Integer limbs: a launch sums at
// most kConstMacTerms products, each at most (q - 1)^2, the carried word and the constant (both below q, together less than one
// product): (T + 1) (q - 1)^2 < 2^128 for the widest prime a context accepts, 2^60.
static_assert(kConstMacTerms + 1 <= (1 << (128 - 2 * kTensorSumPrimeBits)), "const mac sum: the 128-bit accumulator would overflow within one launch");
// fp64 limbs (q < 2^50): the carried word and the constant are below q each, every product is |.| < q, integer-valued doubles are
// exact up to 2^53 >= 8 q: the accumulators are re-centred after every kPlainMacFpTerms = 4 terms (carried + constant + 4 products
// < 6 q, then q/2 + 4 products < 4.5 q), and fp_to_canon centres the last group.
static_assert(kPlainMacFpTerms + 2 <= 8 && kConstMacTerms <= 2 * kPlainMacFpTerms, "const mac sum: the fp64 accumulator would pass 2^53 between two re-centrings");

template <int SIZE>
struct ConstMacLoad {
  u64x2 c[SIZE];
};
template <int SIZE>
__device__ __forceinline__ ConstMacLoad<SIZE> const_mac_load(const u64 *ct, size_t off, size_t pw) {
  ConstMacLoad<SIZE> t;
#pragma unroll
  for (int s = 0; s < SIZE; s++) t.c[s] = *reinterpret_cast<const u64x2 *>(ct + off + s * pw);
  return t;
}
// where this lane's words of term k start: ciphertext `ct`, word w inside a polynomial of term k's own stride
template <int SIZE>
__device__ __forceinline__ size_t const_mac_off(const ConstMacTerms &t, int k, size_t ct, size_t w, int n) {
  return ct * SIZE * ((size_t)t.limbs[k] * n) + w;
}

// one tile on the integers; pc: this lane's words of the carried value, or null
template <int SIZE>
__device__ __forceinline__ void const_mac_int(const ConstMacTerms &t, int nt, int j, const Mod &m, size_t ct, size_t w, int n, size_t pw, const u64 *pc,
                                              u64 *po) {
  U128 ax[SIZE], ay[SIZE];
#pragma unroll
  for (int s = 0; s < SIZE; s++) ax[s] = U128{0, 0}, ay[s] = U128{0, 0};
  if (pc) {  // workgroup-uniform
#pragma unroll
    for (int s = 0; s < SIZE; s++) {
      const u64x2 r = *reinterpret_cast<const u64x2 *>(pc + s * pw);
      ax[s].lo = r.x, ay[s].lo = r.y;
    }
  }
  const u64 cst = t.cst[j];
  add128(ax[0], U128{cst, 0}), add128(ay[0], U128{cst, 0});
  u64 wk[kConstMacTerms];  // every weight of the launch ahead of the loop: the scalar loads are in flight together, not one per term
#pragma unroll
  for (int k = 0; k < kConstMacTerms; k++) wk[k] = t.w[k][j];
  ConstMacLoad<SIZE> cur{}, nxt{};
  if (nt > 0) cur = const_mac_load<SIZE>(t.ct[0], const_mac_off<SIZE>(t, 0, ct, w, n), (size_t)t.limbs[0] * n);
#pragma unroll
  for (int k = 0; k < kConstMacTerms; k++) {
    if (k < nt) {  // workgroup-uniform
      if (k + 1 < kConstMacTerms && k + 1 < nt) nxt = const_mac_load<SIZE>(t.ct[k + 1], const_mac_off<SIZE>(t, k + 1, ct, w, n), (size_t)t.limbs[k + 1] * n);
#pragma unroll
      for (int s = 0; s < SIZE; s++) mac128(ax[s], cur.c[s].x, wk[k]), mac128(ay[s], cur.c[s].y, wk[k]);
      cur = nxt;
    }
  }
  const u64 r64 = reduce64(0ull - m.q, m);  // 2^64 mod q
#pragma unroll
  for (int s = 0; s < SIZE; s++) *reinterpret_cast<u64x2 *>(po + s * pw) = u64x2{reduce128(ax[s], r64, m), reduce128(ay[s], r64, m)};
}

// one tile in fp64 (q < 2^50)
template <int SIZE>
__device__ __forceinline__ void const_mac_fp(const ConstMacTerms &t, int nt, int j, const Mod &m, size_t ct, size_t w, int n, size_t pw, const u64 *pc,
                                             u64 *po) {
  const double q = m.qd, qinv = m.qinv;
  double ax[SIZE], ay[SIZE];
#pragma unroll
  for (int s = 0; s < SIZE; s++) ax[s] = 0, ay[s] = 0;
  if (pc) {  // workgroup-uniform
#pragma unroll
    for (int s = 0; s < SIZE; s++) {
      const u64x2 r = *reinterpret_cast<const u64x2 *>(pc + s * pw);
      ax[s] = fp_from_u64(r.x), ay[s] = fp_from_u64(r.y);
    }
  }
  const double cst = fp_from_u64(t.cst[j]);
  ax[0] += cst, ay[0] += cst;
  double wk[kConstMacTerms];  // every weight of the launch ahead of the loop, converted once
#pragma unroll
  for (int k = 0; k < kConstMacTerms; k++) wk[k] = fp_from_u64(t.w[k][j]);
  ConstMacLoad<SIZE> cur{}, nxt{};
  if (nt > 0) cur = const_mac_load<SIZE>(t.ct[0], const_mac_off<SIZE>(t, 0, ct, w, n), (size_t)t.limbs[0] * n);
#pragma unroll
  for (int k = 0; k < kConstMacTerms; k++) {
    if (k < nt) {  // workgroup-uniform
      if (k + 1 < kConstMacTerms && k + 1 < nt) nxt = const_mac_load<SIZE>(t.ct[k + 1], const_mac_off<SIZE>(t, k + 1, ct, w, n), (size_t)t.limbs[k + 1] * n);
#pragma unroll
      for (int s = 0; s < SIZE; s++) {
        ax[s] += fp_mulmod(fp_from_u64(cur.c[s].x), wk[k], q, qinv);
        ay[s] += fp_mulmod(fp_from_u64(cur.c[s].y), wk[k], q, qinv);
      }
      // carried value + constant + kPlainMacFpTerms products < 6 q < 2^53 up to here
      if ((k + 1) % kPlainMacFpTerms == 0 && k + 1 < kConstMacTerms) {
#pragma unroll
        for (int s = 0; s < SIZE; s++) ax[s] = fp_centre(ax[s], q, qinv), ay[s] = fp_centre(ay[s], q, qinv);
      }
      cur = nxt;
    }
  }
#pragma unroll
  for (int s = 0; s < SIZE; s++) *reinterpret_cast<u64x2 *>(po + s * pw) = u64x2{fp_to_canon(ax[s], q, qinv), fp_to_canon(ay[s], q, qinv)};
}

// tiles, fpmask, HAS_FP / HAS_INT as in k_ckks_plain_mac_sum; nt may be 0 (carry + constant); carry: [count][SIZE][nl][N] like out
// (and possibly out itself), or null
template <bool HAS_FP, bool HAS_INT, int SIZE>
__global__ __launch_bounds__(256) void k_ckks_const_mac_sum(DevCtx c, ConstMacTerms t, int nt, const u64 *carry, u64 *out, int nl, size_t tiles,
                                                            u32 fpmask) {
  const u32 spans = (u32)c.n / kTensorSumSpan;
  const size_t pw = (size_t)nl * c.n;
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t limb = tile / spans;  // ct * nl + j
    const u32 span = (u32)(tile - limb * spans);
    const size_t ct = limb / (u32)nl;
    const int j = (int)(limb - ct * (u32)nl);
    const size_t w = (size_t)j * c.n + (size_t)span * kTensorSumSpan + 2 * threadIdx.x;  // word inside a polynomial, whatever its stride
    const Mod m = mod_at(c, j);
    const size_t out_off = ct * SIZE * pw + w;
    const u64 *pc = carry ? carry + out_off : nullptr;
    if (HAS_FP && (!HAS_INT || ((fpmask >> j) & 1u))) const_mac_fp<SIZE>(t, nt, j, m, ct, w, c.n, pw, pc, out + out_off);
    else const_mac_int<SIZE>(t, nt, j, m, ct, w, c.n, pw, pc, out + out_off);
  }
}

// out [count][size][nl][N] = (addend or 0) + cst (component 0) + sum over k < n_terms of w[k] * ct[k]; ct: HOST array of device
// pointers, term k [count][size][ct_nl[k]][N] with ct_nl[k] >= nl (ct_nl null: all nl); w: [n_terms][nl] canonical words, cst: [nl]
// or null; n_terms >= 0 (an empty sum is one launch that writes addend + cst), size 2 or 3, on stream c->stream
int launch_ckks_const_mac_sum(abc_hip_ctx *c, const u64 *const *ct, const int *ct_nl, const u64 *w, int n_terms, const u64 *cst, const u64 *addend,
                              u64 *out, int size, int nl, size_t count) {
  const size_t tiles = count * nl * ((size_t)c->n / kTensorSumSpan);
  if (!tiles || n_terms < 0) return 0;
  const u32 full = (1u << nl) - 1u;
  const u32 fpmask = (c->use_fp && (c->facts.data_fp(nl) || !c->sw.no_mixed)) ? c->facts.fp_data_mask(nl) : 0u;
  const size_t cap = 256 * 8 * 16;  // workgroups: every CU several times over, the tile loop beyond
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
  for (int k0 = 0; k0 == 0 || k0 < n_terms; k0 += kConstMacTerms) {
    const int nt = n_terms - k0 < kConstMacTerms ? n_terms - k0 : kConstMacTerms;
    ConstMacTerms t{};
    for (int k = 0; k < kConstMacTerms; k++) {  // unused slots repeat a valid term (none is read)
      const int src = k0 + (k < nt ? k : 0);
      t.ct[k] = nt ? ct[src] : nullptr;
      t.limbs[k] = (u32)(nt && ct_nl ? ct_nl[src] : nl);
      for (int j = 0; j < nl; j++) t.w[k][j] = k < nt ? w[(size_t)src * nl + j] : 0;
    }
    for (int j = 0; j < nl; j++) t.cst[j] = (cst && !k0) ? cst[j] : 0;
    const u64 *carry = k0 ? out : addend;
    auto go = [&](auto has_fp, auto has_int, auto sz) {
      hipLaunchKernelGGL((k_ckks_const_mac_sum<decltype(has_fp)::value, decltype(has_int)::value, decltype(sz)::value>), grid, dim3(256), 0,
                         c->stream, c->dc, t, nt, carry, out, nl, tiles, fpmask);
    };
    auto by_size = [&](auto has_fp, auto has_int) {
      if (size == 3) go(has_fp, has_int, std::integral_constant<int, 3>{});
      else go(has_fp, has_int, std::integral_constant<int, 2>{});
    };
    if (fpmask == full) by_size(std::true_type{}, std::false_type{});
    else if (!fpmask) by_size(std::false_type{}, std::true_type{});
    else by_size(std::true_type{}, std::true_type{});
    ABC_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// ---- K-term plaintext sum + rescale in one: carry + sum_k plain_k (.) ct_k formed in the loads of R1 and R2 ----
// The K-term forms of k_mulplain_rescale_intt_fp / _mixed / _ntt above: what enters R1's inverse transform is the dropped limb of
// (carry or 0) + sum over the launch's terms of plain_k (.) ct_k, and the same expression per limb j enters R2's diff_mul_fwd in place
// of x[i].  The term pointers travel by value as in k_ckks_plain_mac_sum (indexed by constants only: the loop is unrolled), carry is
// [count][size][nl][N] like a term's ciphertext, or null.  One functor per arithmetic forms the sums, kStage / kChunk coefficients of
// a lane at a time with the loop over the terms OUTSIDE the one over the coefficients: a term's 2 * kChunk loads are in flight together
// (coefficient by coefficient, the workgroup-uniform branch per term left two).  R1 stages its limb in the transform's LDS before
// the transform, by coalesced loads (plain_sum_stage); R2 forms the sums behind its transform (divround_finish's XL).  The sum is
// exact modulo q whatever its representative, so the result is bit-identical to k_ckks_plain_mac_sum followed by the rescale kernels.
// fp64 (q < 2^50): the arithmetic of plain_mac_fp -- the carried word is below q, every product |.| < q, a re-centring after every
// kPlainMacFpTerms products (carried + 4 products < 5 q, then q/2 + 4 products < 4.5 q; 1 + kPlainMacTerms products would pass
// 8 q <= 2^53), and one more at the end: |result| <= q/2, inside the |.| < q that FpArith::mul_u64 hands to the same consumers.
static_assert(kPlainMacFpTerms + 1 <= 8 && kPlainMacTerms <= 2 * kPlainMacFpTerms,
              "plain sum rescale: the fp64 accumulator would pass 2^53 between two re-centrings");
struct PlainSumLimbFp {
  static constexpr int kStage = 16, kChunk = 4;  // coefficients at a time: R1 (nothing else is live), R2 (beside the transform's sixteen outputs)
  const PlainMacTerms &t;
  int nt;
  const u64 *__restrict__ carry;  // this limb of the carried value, or null
  size_t ct_off, plain_off;       // of this limb inside a term's ciphertext / plaintext
  double q, qinv;
  template <int C>
  __device__ __forceinline__ void sums(const int (&i)[C], double (&out)[C]) const {
    double acc[C];
#pragma unroll
    for (int e = 0; e < C; e++) acc[e] = 0.0;
    if (carry) {  // workgroup-uniform
#pragma unroll
      for (int e = 0; e < C; e++) acc[e] = fp_from_u64(carry[i[e]]);
    }
#pragma unroll
    for (int k = 0; k < kPlainMacTerms; k++) {
      if (k < nt) {  // workgroup-uniform
        const u64 *__restrict__ ct = t.ct[k] + ct_off, *__restrict__ pl = t.plain[k] + plain_off;
        u64 cv[C], pv[C];
#pragma unroll
        for (int e = 0; e < C; e++) cv[e] = ct[i[e]], pv[e] = pl[i[e]];
#pragma unroll
        for (int e = 0; e < C; e++) acc[e] += fp_mulmod(fp_from_u64(cv[e]), fp_from_u64(pv[e]), q, qinv);
        if ((k + 1) % kPlainMacFpTerms == 0 && k + 1 < kPlainMacTerms) {
#pragma unroll
          for (int e = 0; e < C; e++) acc[e] = fp_centre(acc[e], q, qinv);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < C; e++) out[e] = fp_centre(acc[e], q, qinv);
  }
};
// integers: the arithmetic of plain_mac_int -- (kPlainMacTerms + 1) (q - 1)^2 < 2^128 for the widest prime a context accepts (the
// static_assert beside PlainMacTerms), one reduction: canonical, what IntArith::mul_u64 returns.  Eight coefficients at a time in
// R1: their 128-bit accumulators and a term's loads are 64 VGPRs.
struct PlainSumLimbInt {
  static constexpr int kStage = 8, kChunk = 2;
  const PlainMacTerms &t;
  int nt;
  const u64 *__restrict__ carry;
  size_t ct_off, plain_off;
  Mod m;
  template <int C>
  __device__ __forceinline__ void sums(const int (&i)[C], u64 (&out)[C]) const {
    U128 acc[C];
#pragma unroll
    for (int e = 0; e < C; e++) acc[e] = U128{0, 0};
    if (carry) {  // workgroup-uniform
#pragma unroll
      for (int e = 0; e < C; e++) acc[e].lo = carry[i[e]];
    }
#pragma unroll
    for (int k = 0; k < kPlainMacTerms; k++) {
      if (k < nt) {  // workgroup-uniform
        const u64 *__restrict__ ct = t.ct[k] + ct_off, *__restrict__ pl = t.plain[k] + plain_off;
        u64 cv[C], pv[C];
#pragma unroll
        for (int e = 0; e < C; e++) cv[e] = ct[i[e]], pv[e] = pl[i[e]];
#pragma unroll
        for (int e = 0; e < C; e++) mac128(acc[e], cv[e], pv[e]);
      }
    }
    const u64 r64 = reduce64(0ull - m.q, m);  // 2^64 mod q
#pragma unroll
    for (int e = 0; e < C; e++) out[e] = reduce128(acc[e], r64, m);
  }
};
__device__ __forceinline__ PlainSumLimbFp plain_sum_limb_fp(const PlainMacTerms &t, int nt, const u64 *carry, size_t ct_off, size_t plain_off,
                                                            const Mod &m) {
  return PlainSumLimbFp{t, nt, carry ? carry + ct_off : nullptr, ct_off, plain_off, m.qd, m.qinv};
}
__device__ __forceinline__ PlainSumLimbInt plain_sum_limb_int(const PlainMacTerms &t, int nt, const u64 *carry, size_t ct_off, size_t plain_off,
                                                              const Mod &m) {
  return PlainSumLimbInt{t, nt, carry ? carry + ct_off : nullptr, ct_off, plain_off, m};
}
// R1: the limb's N sums into the transform's LDS, lane `tid` those of the coefficients tid + e * (N / 16) (coalesced), then the
// barrier; the transform's first pass reads word lds_pad(i) for coefficient i (LdsOperand) and writes back exactly the words it read
template <int LB, class XL, class E>
__device__ __forceinline__ void plain_sum_stage(E *lds, const XL &xl) {
  constexpr int T = (1 << LB) / 16, C = XL::kStage;
#pragma unroll
  for (int c0 = 0; c0 < 16; c0 += C) {
    int ii[C];
    E xs[C];
#pragma unroll
    for (int e = 0; e < C; e++) ii[e] = (int)threadIdx.x + (c0 + e) * T;
    xl.sums(ii, xs);
#pragma unroll
    for (int e = 0; e < C; e++) lds[lds_pad(ii[e])] = xs[e];
  }
  if constexpr (LB <= 10) wave_sync(); else block_sync_lds();
}
template <class E>
struct LdsOperand {
  const E *lds;
  __device__ __forceinline__ E operator()(int i) const { return lds[lds_pad(i)]; }
};

template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_plainsum_rescale_intt_fp(DevCtx c, PlainMacTerms t, int nt, size_t plain_stride,
                                                                             const u64 *__restrict__ carry, u64 *__restrict__ last, int size, int nl) {
  __shared__ double lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB, p = blockIdx.x;
  const Mod m = mod_at(c, nl - 1);
  plain_sum_stage<LB>(lds, plain_sum_limb_fp(t, nt, carry, (p * nl + (nl - 1)) * N, (p / size) * plain_stride + (size_t)(nl - 1) * N, m));
  divround_to_coef<LB, FpArith, false, LdsOperand<double>>(lds, m, fp_table(c, nl - 1), nullptr, last + p * N, nullptr, LdsOperand<double>{lds});
}
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_plainsum_rescale_intt_mixed(DevCtx c, PlainMacTerms t, int nt, size_t plain_stride,
                                                                                const u64 *__restrict__ carry, u64 *__restrict__ last, int size, int nl,
                                                                                int fp_last) {
  __shared__ u64 lds_raw[lds_words(LB)];
  const size_t N = (size_t)1 << LB, p = blockIdx.x;
  const size_t ct_off = (p * nl + (nl - 1)) * N, plain_off = (p / size) * plain_stride + (size_t)(nl - 1) * N;
  u64 *__restrict__ dst = last + p * N;
  if (fp_last) {
    const Mod m = mod_at(c, nl - 1);
    double *lds = reinterpret_cast<double *>(lds_raw);
    plain_sum_stage<LB>(lds, plain_sum_limb_fp(t, nt, carry, ct_off, plain_off, m));
    divround_to_coef<LB, FpArith, false, LdsOperand<double>>(lds, m, fp_table(c, nl - 1), nullptr, dst, nullptr, LdsOperand<double>{lds});
  } else {
    const Mod m = c.mods[nl - 1];
    plain_sum_stage<LB>(lds_raw, plain_sum_limb_int(t, nt, carry, ct_off, plain_off, m));
    divround_to_coef<LB, IntArith<true>, false, LdsOperand<u64>>(lds_raw, m, ntt_table(c, nl - 1), nullptr, dst, nullptr, LdsOperand<u64>{lds_raw});
  }
}
template <int LB, bool MIXED>
__global__ __launch_bounds__((1 << LB) / 16) void k_plainsum_rescale_ntt(DevCtx c, PlainMacTerms t, int nt, size_t plain_stride,
                                                                         const u64 *__restrict__ carry, const u64 *__restrict__ last,
                                                                         u64 *__restrict__ out, int size, int nl, int npoly, u32 fpmask) {
  __shared__ u64 lds_raw[lds_words(LB)];
  int j;
  size_t p;
  xcd_slot(blockIdx.x, nl - 1, npoly, j, p);
  const size_t N = (size_t)1 << LB;
  const Mod m = MIXED ? c.mods[j] : mod_at(c, j);
  const auto fix = round_fix<std::conditional_t<MIXED, u64, double>>(c.mods[nl - 1].q >> 1, m);
  const DropInv d = inv_qlast_at(c, nl - 1, j);
  const u64 *__restrict__ src = last + p * N;
  const size_t ct_off = (p * nl + j) * N, plain_off = (p / size) * plain_stride + (size_t)j * N;
  u64 *__restrict__ o = out + (p * (nl - 1) + j) * N;
  if constexpr (!MIXED) {
    divround_finish<LB, FpArith, false, false, false, PlainSumLimbFp>(reinterpret_cast<double *>(lds_raw), m, fp_table(c, j), fix, d, src, nullptr, nullptr, o,
                                                                      nullptr, plain_sum_limb_fp(t, nt, carry, ct_off, plain_off, m));
  } else if ((fpmask >> j) & 1u) {
    const Mod mf = mod_at(c, j);
    divround_finish<LB, FpArith, true, false, false, PlainSumLimbFp>(reinterpret_cast<double *>(lds_raw), mf, fp_table(c, j), fix, d, src, nullptr, nullptr, o,
                                                                     nullptr, plain_sum_limb_fp(t, nt, carry, ct_off, plain_off, mf));
  } else {
    divround_finish<LB, IntArith<true>, false, false, false, PlainSumLimbInt>(lds_raw, m, ntt_table(c, j), fix, d, src, nullptr, nullptr, o, nullptr,
                                                                              plain_sum_limb_int(t, nt, carry, ct_off, plain_off, m));
  }
}
template <int LB, bool MIXED>
static int launch_plain_sum_rescale_lds(abc_hip_ctx *c, const PlainMacTerms &t, int nt, size_t plain_stride, const u64 *carry, u64 *out, int size, int nl,
                                        size_t polys, u32 fpmask) {
  const size_t N = (size_t)1 << LB;
  if (ensure_workspace(c, polys * N * 8)) return 1;
  u64 *last = (u64 *)c->ws;
  const dim3 block((1 << LB) / 16);
  if constexpr (MIXED)
    hipLaunchKernelGGL(k_plainsum_rescale_intt_mixed<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, t, nt, plain_stride, carry, last, size, nl,
                       (int)((fpmask >> (nl - 1)) & 1u));
  else
    hipLaunchKernelGGL(k_plainsum_rescale_intt_fp<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, t, nt, plain_stride, carry, last, size, nl);
  hipLaunchKernelGGL((k_plainsum_rescale_ntt<LB, MIXED>), dim3((unsigned)(polys * (nl - 1))), block, 0, c->stream, c->dc, t, nt, plain_stride, carry,
                     last, out, size, nl, (int)polys, fpmask);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// out [count][size][nl-1][N] = rescale((carry or 0) + sum over k < n_terms of plain[k] (.) ct[k]) by the fused pair; the route r is not
// generic, 0 <= n_terms <= kPlainMacTerms with a carry where n_terms is 0, nl >= 2 (plain_sum_rescale in abc_context.hip sees to all three)
int launch_plain_sum_rescale(abc_hip_ctx *c, const RescaleRoute &r, const u64 *const *ct, const u64 *const *plain, size_t plain_stride, int n_terms,
                             const u64 *carry, u64 *out, int size, int nl, size_t count) {
  const size_t polys = count * size;
  if (!polys) return 0;
  if (r.kind == Rescale::generic || n_terms < 0 || n_terms > kPlainMacTerms || (!n_terms && !carry) || nl < 2) {
    set_error("plain_sum_rescale: not a launch of the fused pair");
    return 1;
  }
  PlainMacTerms t;  // unused slots repeat a valid pointer (the carry where there is no term: no slot is read then)
  for (int k = 0; k < kPlainMacTerms; k++) t.ct[k] = n_terms ? ct[k < n_terms ? k : 0] : carry, t.plain[k] = n_terms ? plain[k < n_terms ? k : 0] : carry;
  if (r.kind == Rescale::mixed)
    return dispatch_logn<10, 14>(c->logn, [&](auto LB) {
      return launch_plain_sum_rescale_lds<decltype(LB)::value, true>(c, t, n_terms, plain_stride, carry, out, size, nl, polys, r.fpmask);
    });
  return dispatch_logn<10, 14>(c->logn, [&](auto LB) {
    return launch_plain_sum_rescale_lds<decltype(LB)::value, false>(c, t, n_terms, plain_stride, carry, out, size, nl, polys, 0u);
  });
}

// ---- K-term SCALAR-weighted sum + rescale in one: carry + const + sum_k w_k * ct_k formed in the loads of R1 and R2 ----
// k_plainsum_rescale_* with a functor whose weight is the workgroup-uniform scalar instead of a loaded plaintext word: a term costs
// one load per coefficient, not two.  At most kConstSumRescaleTerms = 4 terms (beyond four the streaming kernel and the rescale are
// as fast: profiles/const_sum_ab.log), every term at level nl -- a term held higher has another stride and stays with
// k_ckks_const_mac_sum.  The record travels by value; the functor is built once per workgroup and holds this limb's weights and
// constant as VALUES (scalar loads from the kernel-argument segment, the limb is workgroup-uniform).  The constant belongs to
// component 0: polynomial p of the batch is component p % size.  Bounds: fp64, carried + constant + 4 products < 6 q < 2^53, one
// centring at the end, |result| <= q/2; integers, (4 + 1) (q - 1)^2 < 2^128, one reduction, canonical.  Exact modular sums whatever
// the representative: bit-identical to k_ckks_const_mac_sum followed by the rescale kernels.
struct ConstSumRescaleTerms {
  const u64 *ct[kConstSumRescaleTerms];
  u64 w[kConstSumRescaleTerms][kMaxLimbs];
  u64 cst[kMaxLimbs];  // zeros where there is no constant
};
static_assert(kConstSumRescaleTerms + 2 <= 8, "const sum rescale: the fp64 accumulator would pass 2^53 before its one centring");
static_assert(kConstSumRescaleTerms + 1 <= (1 << (128 - 2 * kTensorSumPrimeBits)), "const sum rescale: the 128-bit accumulator would overflow");
// CHUNK: coefficients R2 asks for at a time behind its transform (kChunk); the mixed R2 kernel at N = 2^14 -- 1024 threads, 128 VGPRs
// at most -- takes half of what its twins take, which keeps it out of scratch
template <int CHUNK>
struct ConstSumLimbFpT {
  static constexpr int kStage = 16, kChunk = CHUNK;
  const u64 *ct[kConstSumRescaleTerms];  // this limb of every term
  int nt;
  const u64 *__restrict__ carry;  // this limb of the carried value, or null
  u64 w[kConstSumRescaleTerms], cst;  // canonical words: uniform, so they stay in scalar registers across the transform; converted at each use
  double q, qinv;
  template <int C>
  __device__ __forceinline__ void sums(const int (&i)[C], double (&out)[C]) const {
    double acc[C];
    const double c0 = fp_from_u64(cst);
#pragma unroll
    for (int e = 0; e < C; e++) acc[e] = c0;
    if (carry) {  // workgroup-uniform
#pragma unroll
      for (int e = 0; e < C; e++) acc[e] += fp_from_u64(carry[i[e]]);
    }
#pragma unroll
    for (int k = 0; k < kConstSumRescaleTerms; k++) {
      if (k < nt) {  // workgroup-uniform
        u64 cv[C];
#pragma unroll
        for (int e = 0; e < C; e++) cv[e] = ct[k][i[e]];
        const double wk = fp_from_u64(w[k]);
#pragma unroll
        for (int e = 0; e < C; e++) acc[e] += fp_mulmod(fp_from_u64(cv[e]), wk, q, qinv);
      }
    }
#pragma unroll
    for (int e = 0; e < C; e++) out[e] = fp_centre(acc[e], q, qinv);
  }
};
template <int CHUNK>
struct ConstSumLimbIntT {
  static constexpr int kStage = 8, kChunk = CHUNK;
  const u64 *ct[kConstSumRescaleTerms];
  int nt;
  const u64 *__restrict__ carry;
  u64 w[kConstSumRescaleTerms], cst;
  Mod m;
  template <int C>
  __device__ __forceinline__ void sums(const int (&i)[C], u64 (&out)[C]) const {
    U128 acc[C];
#pragma unroll
    for (int e = 0; e < C; e++) acc[e] = U128{cst, 0};
    if (carry) {  // workgroup-uniform
#pragma unroll
      for (int e = 0; e < C; e++) add128(acc[e], U128{carry[i[e]], 0});
    }
#pragma unroll
    for (int k = 0; k < kConstSumRescaleTerms; k++) {
      if (k < nt) {  // workgroup-uniform
        u64 cv[C];
#pragma unroll
        for (int e = 0; e < C; e++) cv[e] = ct[k][i[e]];
#pragma unroll
        for (int e = 0; e < C; e++) mac128(acc[e], cv[e], w[k]);
      }
    }
    const u64 r64 = reduce64(0ull - m.q, m);  // 2^64 mod q
#pragma unroll
    for (int e = 0; e < C; e++) out[e] = reduce128(acc[e], r64, m);
  }
};
using ConstSumLimbFp = ConstSumLimbFpT<4>;
using ConstSumLimbInt = ConstSumLimbIntT<2>;
// limb j of polynomial p (component p % size): off = (p * nl + j) * N
template <class F = ConstSumLimbFp>
__device__ __forceinline__ F const_sum_limb_fp(const ConstSumRescaleTerms &t, int nt, const u64 *carry, size_t off, int j, bool comp0, const Mod &m) {
  F f;
#pragma unroll
  for (int k = 0; k < kConstSumRescaleTerms; k++) f.ct[k] = t.ct[k] + off, f.w[k] = t.w[k][j];
  f.nt = nt, f.carry = carry ? carry + off : nullptr, f.cst = comp0 ? t.cst[j] : 0, f.q = m.qd, f.qinv = m.qinv;
  return f;
}
template <class F = ConstSumLimbInt>
__device__ __forceinline__ F const_sum_limb_int(const ConstSumRescaleTerms &t, int nt, const u64 *carry, size_t off, int j, bool comp0, const Mod &m) {
  F f;
#pragma unroll
  for (int k = 0; k < kConstSumRescaleTerms; k++) f.ct[k] = t.ct[k] + off, f.w[k] = t.w[k][j];
  f.nt = nt, f.carry = carry ? carry + off : nullptr, f.cst = comp0 ? t.cst[j] : 0, f.m = m;
  return f;
}

// LdsOperand under a name of its own: divround_to_coef<.., ScalarLdsOperand<E>> is then an instantiation of its own, and the ones the
// k_plainsum_rescale_* kernels call keep the callers -- and with them the inlining and the device code -- they had
template <class E>
struct ScalarLdsOperand {
  const E *lds;
  __device__ __forceinline__ E operator()(int i) const { return lds[lds_pad(i)]; }
};
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_constsum_rescale_intt_fp(DevCtx c, ConstSumRescaleTerms t, int nt, const u64 *__restrict__ carry,
                                                                             u64 *__restrict__ last, int size, int nl) {
  __shared__ double lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB, p = blockIdx.x;
  const Mod m = mod_at(c, nl - 1);
  plain_sum_stage<LB>(lds, const_sum_limb_fp(t, nt, carry, (p * nl + (nl - 1)) * N, nl - 1, p % size == 0, m));
  divround_to_coef<LB, FpArith, false, ScalarLdsOperand<double>>(lds, m, fp_table(c, nl - 1), nullptr, last + p * N, nullptr, ScalarLdsOperand<double>{lds});
}
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_constsum_rescale_intt_mixed(DevCtx c, ConstSumRescaleTerms t, int nt, const u64 *__restrict__ carry,
                                                                                u64 *__restrict__ last, int size, int nl, int fp_last) {
  __shared__ u64 lds_raw[lds_words(LB)];
  const size_t N = (size_t)1 << LB, p = blockIdx.x;
  const size_t off = (p * nl + (nl - 1)) * N;
  const bool comp0 = p % size == 0;
  u64 *__restrict__ dst = last + p * N;
  if (fp_last) {
    const Mod m = mod_at(c, nl - 1);
    double *lds = reinterpret_cast<double *>(lds_raw);
    plain_sum_stage<LB>(lds, const_sum_limb_fp(t, nt, carry, off, nl - 1, comp0, m));
    divround_to_coef<LB, FpArith, false, ScalarLdsOperand<double>>(lds, m, fp_table(c, nl - 1), nullptr, dst, nullptr, ScalarLdsOperand<double>{lds});
  } else {
    const Mod m = c.mods[nl - 1];
    plain_sum_stage<LB>(lds_raw, const_sum_limb_int(t, nt, carry, off, nl - 1, comp0, m));
    divround_to_coef<LB, IntArith<true>, false, ScalarLdsOperand<u64>>(lds_raw, m, ntt_table(c, nl - 1), nullptr, dst, nullptr, ScalarLdsOperand<u64>{lds_raw});
  }
}
template <int LB, bool MIXED>
__global__ __launch_bounds__((1 << LB) / 16) void k_constsum_rescale_ntt(DevCtx c, ConstSumRescaleTerms t, int nt, const u64 *__restrict__ carry,
                                                                         const u64 *__restrict__ last, u64 *__restrict__ out, int size, int nl, int npoly,
                                                                         u32 fpmask) {
  __shared__ u64 lds_raw[lds_words(LB)];
  int j;
  size_t p;
  xcd_slot(blockIdx.x, nl - 1, npoly, j, p);
  const size_t N = (size_t)1 << LB;
  const Mod m = MIXED ? c.mods[j] : mod_at(c, j);
  const auto fix = round_fix<std::conditional_t<MIXED, u64, double>>(c.mods[nl - 1].q >> 1, m);
  const DropInv d = inv_qlast_at(c, nl - 1, j);
  const u64 *__restrict__ src = last + p * N;
  const size_t off = (p * nl + j) * N;
  const bool comp0 = p % size == 0;
  u64 *__restrict__ o = out + (p * (nl - 1) + j) * N;
  if constexpr (!MIXED) {
    divround_finish<LB, FpArith, false, false, false, ConstSumLimbFp>(reinterpret_cast<double *>(lds_raw), m, fp_table(c, j), fix, d, src, nullptr, nullptr, o,
                                                                      nullptr, const_sum_limb_fp(t, nt, carry, off, j, comp0, m));
  } else {
    using Fp = std::conditional_t<LB == 14, ConstSumLimbFpT<2>, ConstSumLimbFp>;
    using Int = std::conditional_t<LB == 14, ConstSumLimbIntT<1>, ConstSumLimbInt>;
    if ((fpmask >> j) & 1u) {
      const Mod mf = mod_at(c, j);
      divround_finish<LB, FpArith, true, false, false, Fp>(reinterpret_cast<double *>(lds_raw), mf, fp_table(c, j), fix, d, src, nullptr, nullptr, o, nullptr,
                                                           const_sum_limb_fp<Fp>(t, nt, carry, off, j, comp0, mf));
    } else {
      divround_finish<LB, IntArith<true>, false, false, false, Int>(lds_raw, m, ntt_table(c, j), fix, d, src, nullptr, nullptr, o, nullptr,
                                                                    const_sum_limb_int<Int>(t, nt, carry, off, j, comp0, m));
    }
  }
}
template <int LB, bool MIXED>
static int launch_const_sum_rescale_lds(abc_hip_ctx *c, const ConstSumRescaleTerms &t, int nt, const u64 *carry, u64 *out, int size, int nl, size_t polys,
                                        u32 fpmask) {
  const size_t N = (size_t)1 << LB;
  if (ensure_workspace(c, polys * N * 8)) return 1;
  u64 *last = (u64 *)c->ws;
  const dim3 block((1 << LB) / 16);
  if constexpr (MIXED)
    hipLaunchKernelGGL(k_constsum_rescale_intt_mixed<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, t, nt, carry, last, size, nl,
                       (int)((fpmask >> (nl - 1)) & 1u));
  else
    hipLaunchKernelGGL(k_constsum_rescale_intt_fp<LB>, dim3((unsigned)polys), block, 0, c->stream, c->dc, t, nt, carry, last, size, nl);
  hipLaunchKernelGGL((k_constsum_rescale_ntt<LB, MIXED>), dim3((unsigned)(polys * (nl - 1))), block, 0, c->stream, c->dc, t, nt, carry, last, out, size, nl,
                     (int)polys, fpmask);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

// out [count][size][nl-1][N] = rescale((addend or 0) + cst (component 0) + sum over k < n_terms of w[k] * ct[k]) by the fused pair; every
// term at nl limbs, 1 <= n_terms <= kConstSumRescaleTerms, r not generic, nl >= 2 (const_sum_rescale in abc_context.hip sees to it)
int launch_const_sum_rescale(abc_hip_ctx *c, const RescaleRoute &r, const u64 *const *ct, const u64 *w, int n_terms, const u64 *cst, const u64 *addend,
                             u64 *out, int size, int nl, size_t count) {
  const size_t polys = count * size;
  if (!polys) return 0;
  if (r.kind == Rescale::generic || n_terms < 1 || n_terms > kConstSumRescaleTerms || nl < 2) {
    set_error("const_sum_rescale: not a launch of the fused pair");
    return 1;
  }
  ConstSumRescaleTerms t{};  // unused slots repeat a valid pointer (none is read)
  for (int k = 0; k < kConstSumRescaleTerms; k++) {
    t.ct[k] = ct[k < n_terms ? k : 0];
    for (int j = 0; j < nl; j++) t.w[k][j] = k < n_terms ? w[(size_t)k * nl + j] : 0;
  }
  for (int j = 0; j < nl; j++) t.cst[j] = cst ? cst[j] : 0;
  if (r.kind == Rescale::mixed)
    return dispatch_logn<10, 14>(c->logn, [&](auto LB) {
      return launch_const_sum_rescale_lds<decltype(LB)::value, true>(c, t, n_terms, addend, out, size, nl, polys, r.fpmask);
    });
  return dispatch_logn<10, 14>(c->logn, [&](auto LB) {
    return launch_const_sum_rescale_lds<decltype(LB)::value, false>(c, t, n_terms, addend, out, size, nl, polys, 0u);
  });
}

}  // namespace abc
