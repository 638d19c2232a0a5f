// abc_kernels_fused.hip -- the hot path for N <= 2^14 (one workgroup per RNS limb, the limb resident in LDS):
// hybrid key switching for relinearisation and Galois rotations (BFV and CKKS) and the CKKS
// ciphertext x ciphertext multiply + relinearise front end.
//
// Replaces, for rings that fit LDS:
//   SealCiphertext::multiply / multiplyInplace = Evaluator::multiply + relinearize_inplace
//       (src/runtime/SealCiphertext.cpp:102-107,121-124)                     -> launch_mul_relin, launch_keyswitch
//   SealCiphertext::rotateRows / rotateRowsInplace = Evaluator::rotate_rows    (:52-61) -> launch_keyswitch
// Which sequence a call takes -- the split fp64 kernels at N = 2^14, the LDS-resident fp64 or integer kernels, or one of the
// other translation units' -- is decided in abc_route.hpp and tabulated in DESIGN.md section 3b; the launch functions at the end
// of this file switch over that route.  tests/test_gpu_paths.py holds every route bit-identical to the oracle.
// The operand transform and the decomposition are templates over the arithmetic policy (IntArith<GUARD> / FpArith, abc_ntt.hpp),
// whose element operations spell the loads and stores around a transform; the integer mod-down is abc_ntt.hpp's "divide and
// round" step B.  The other mod-down kernels keep one kernel per arithmetic ("Where the twins stay", above K2c).
// Algorithmic HBM bytes per multiply: 8N(6L + 2L(L+1)); measured: DESIGN.md section 4.
#include <type_traits>

#include "abc_context.hpp"
#include "abc_host_math.hpp"

namespace abc {

// ---------------------------------------------------------------------------------------------------------------
// K1 (CKKS multiply front end)
// ---------------------------------------------------------------------------------------------------------------
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_tensor_intt(DevCtx c, const u64 *__restrict__ a,
                                                                      const u64 *__restrict__ b, u64 *__restrict__ c01,
                                                                      u64 *__restrict__ c2coef, u64 *__restrict__ c2ntt, int nl) {
  __shared__ u64 lds[lds_words(LB)];
  const int j = blockIdx.x % nl;
  const size_t ct = blockIdx.x / nl;
  const size_t N = (size_t)1 << LB, pw = (size_t)nl * N;
  const Mod m = c.mods[j];
  const NttTable t = ntt_table(c, j);
  const u64 *__restrict__ a0 = a + ct * 2 * pw + j * N, *__restrict__ a1 = a0 + pw;
  const u64 *__restrict__ b0 = b + ct * 2 * pw + j * N, *__restrict__ b1 = b0 + pw;
  u64 *__restrict__ o0 = c01 + ct * 2 * pw + j * N, *__restrict__ o1 = o0 + pw;
  u64 *__restrict__ dcoef = c2coef + (ct * nl + j) * N, *__restrict__ dntt = c2ntt + (ct * nl + j) * N;
  ntt_inv_block<LB>(
      lds,
      [&](int, int i) {
        const u64 x0 = a0[i], x1 = a1[i], y0 = b0[i], y1 = b1[i];
        o0[i] = mul_mod(x0, y0, m);
        U128 acc = mul_wide(x0, y1);
        mac128(acc, x1, y0);
        o1[i] = barrett_reduce(acc, m);
        const u64 v = mul_mod(x1, y1, m);
        dntt[i] = v;
        return v;
      },
      [&](int, int i, u64 v) { dcoef[i] = scale_inv_n(v, m); }, t, m, 0, 0);
}

// The next two kernels are written once over the arithmetic policy A (abc_ntt.hpp): IntArith<GUARD>, or FpArith when every key
// prime is below 2^50.  Same buffers, same u64 memory format, bit-identical results; only the arithmetic between the HBM load
// and the HBM store differs, and that is spelt by the policy's element operations.
//
// inverse transform of the key-switch operand when it arrives in NTT form (CKKS rotations):
// src limb (ct, j) at src + ct*src_stride + j*N  ->  dst[ct][j]
template <int LB, class A>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_operand_intt(DevCtx c, const u64 *__restrict__ src, size_t src_stride,
                                                                       u64 *__restrict__ dst, int nl) {
  using E = typename A::E;
  __shared__ E lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB;
  const int j = blockIdx.x % nl;
  const size_t ct = blockIdx.x / nl;
  const Mod m = arith_mod<A>(c, j);
  const typename A::Table t = arith_table<A>(c, j);
  const u64 *__restrict__ s = src + ct * src_stride + (size_t)j * N;
  u64 *__restrict__ d = dst + (size_t)blockIdx.x * N;
  ntt_inv_block_a<LB, A>(
      lds, [&](int, int i) { return A::from_u64(s[i]); }, [&](int, int i, E v) { d[i] = A::canon(A::scale_n(v, m), m); }, t, m, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------
// key switch: operand in coefficient form at coef + ct*coef_stride + J*N; CKKS additionally has the operand's own
// NTT form at ntt + ct*ntt_stride + J*N (used where q_J is the key prime: switch_key_inplace, CKKS branch)
// ---------------------------------------------------------------------------------------------------------------
// K2a: dec[ct][I][J] = NTT_I( operand_J mod q_I )
// LAZY (unguarded transforms over primes <= 55 bits): the transform's raw outputs (< 64q) are stored as they are;
// the inner product accumulates 128-bit products and reduces once, so it needs no canonical operands.  fp64 always stores
// non-negative lazy representatives (A::fwd_out).
template <int LB, class A, bool LAZY>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_decomp_ntt(DevCtx c, const u64 *__restrict__ coef, size_t coef_stride,
                                                                        u64 *__restrict__ dec, int nl, int skip_diagonal) {
  using E = typename A::E;
  __shared__ E lds[lds_words(LB)];
  const int J = blockIdx.x % nl;
  const int I = (blockIdx.x / nl) % (nl + 1);
  const size_t ct = blockIdx.x / ((size_t)nl * (nl + 1));
  if (skip_diagonal && J == I) return;
  const size_t N = (size_t)1 << LB;
  const int ki = (I == nl) ? c.K - 1 : I;
  const Mod m = arith_mod<A>(c, ki);
  const typename A::Table t = arith_table<A>(c, ki);
  const u64 *__restrict__ src = coef + ct * coef_stride + (size_t)J * N;
  u64 *__restrict__ dst = dec + ((ct * (nl + 1) + I) * nl + J) * N;
  // residues are < q_J already: reduced only where the transform would not accept them (A::fwd_accepts; fp64: never).
  // Workgroup-uniform choice between two straight-line bodies, so the sixteen coefficient loads of a lane are issued back to
  // back in either.
  auto st = [&](int, int i, E v) { dst[i] = A::template fwd_out<LAZY>(v, m); };
  if (!A::fwd_accepts(c.mods[J].q, m))
    ntt_fwd_block_a<LB, A>(lds, [&](int, int i) { return A::from_u64(reduce64(src[i], m)); }, st, t, m, 0, 0);
  else
    ntt_fwd_block_a<LB, A>(lds, [&](int, int i) { return A::from_u64(src[i]); }, st, t, m, 0, 0);
}

// K2b: acc_comp[k] = sum_J x_J[k] * key[J][comp][I][k]; data primes -> ksacc[ct][comp][I], special -> tsp[ct][comp]
__global__ __launch_bounds__(256) void k_fused_ks_mac(DevCtx c, const u64 *__restrict__ dec, const u64 *__restrict__ ntt,
                                                      size_t ntt_stride, const u64 *__restrict__ key, u64 *__restrict__ ksacc,
                                                      u64 *__restrict__ tsp, int nl, size_t count) {
  const size_t N = (size_t)c.n;
  const size_t per_ct = (size_t)(nl + 1) * (N / 2);
  const size_t items = count * per_ct;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ct = it / per_ct, r = it % per_ct;
    const int I = (int)(r / (N / 2));
    const size_t k = (r % (N / 2)) * 2;
    const int ki = (I == nl) ? c.K - 1 : I;
    const Mod m = c.mods[ki];
    U128 a00{0, 0}, a01{0, 0}, a10{0, 0}, a11{0, 0};
    for (int J = 0; J < nl; J++) {
      const u64 *xs = (ntt && J == I) ? ntt + ct * ntt_stride + (size_t)J * N + k : dec + ((ct * (nl + 1) + I) * nl + J) * N + k;
      const u64x2 x = *reinterpret_cast<const u64x2 *>(xs);
      const u64x2 k0 = *reinterpret_cast<const u64x2 *>(key + (((size_t)J * 2 + 0) * c.K + ki) * N + k);
      const u64x2 k1 = *reinterpret_cast<const u64x2 *>(key + (((size_t)J * 2 + 1) * c.K + ki) * N + k);
      mac128(a00, x.x, k0.x); mac128(a01, x.y, k0.y);
      mac128(a10, x.x, k1.x); mac128(a11, x.y, k1.y);
      if ((J & 3) == 3 || J == nl - 1) {  // flush: barrett_reduce admits 4 products of reduced operands
        a00 = U128{barrett_reduce(a00, m), 0}; a01 = U128{barrett_reduce(a01, m), 0};
        a10 = U128{barrett_reduce(a10, m), 0}; a11 = U128{barrett_reduce(a11, m), 0};
      }
    }
    u64x2 r0{a00.lo, a01.lo}, r1{a10.lo, a11.lo};
    if (I == nl) {
      *reinterpret_cast<u64x2 *>(tsp + (ct * 2 + 0) * N + k) = r0;
      *reinterpret_cast<u64x2 *>(tsp + (ct * 2 + 1) * N + k) = r1;
    } else {
      *reinterpret_cast<u64x2 *>(ksacc + ((ct * 2 + 0) * nl + I) * N + k) = r0;
      *reinterpret_cast<u64x2 *>(ksacc + ((ct * 2 + 1) * nl + I) * N + k) = r1;
    }
  }
}

// Where the twins stay.  K2c (step A of abc_ntt.hpp's "divide and round") and the fp64 and BFV forms of K3 keep one kernel per
// arithmetic: folded into divround_to_coef / divround_finish or into one template over the policy, some of their instantiations
// came out with other register counts (profiles/r08_divide_round_ab.log), and this file's rule is that a fold may not do that.
// The integer K3 and rescale's kernels (abc_kernels_eval.hip) do share the bodies.
// K2c: special-prime limb back to coefficients, plus q_sp/2 (rounding of the division by q_sp)
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_special_intt(DevCtx c, const u64 *__restrict__ tsp,
                                                                          u64 *__restrict__ tlast) {
  __shared__ u64 lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB;
  const Mod m = c.mods[c.K - 1];
  const NttTable t = ntt_table(c, c.K - 1);
  const u64 half = m.q >> 1;
  const u64 *__restrict__ src = tsp + (size_t)blockIdx.x * N;
  u64 *__restrict__ dst = tlast + (size_t)blockIdx.x * N;
  ntt_inv_block<LB>(
      lds, [&](int, int i) { return src[i]; }, [&](int, int i, u64 v) { dst[i] = add_mod(scale_inv_n(v, m), half, m.q); }, t, m,
      0, 0);
}

// K3, CKKS: out[ct][comp][j] = (ksacc - NTT_j(tlast mod q_j + fix)) * q_sp^-1 (+ addend): step B, abc_ntt.hpp's divround_finish
template <int LB, bool GUARD>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_moddown(DevCtx c, const u64 *__restrict__ ksacc,
                                                                     const u64 *__restrict__ tlast, const u64 *__restrict__ addend,
                                                                     size_t addend_stride, int add_c1, u64 *__restrict__ out, int nl) {
  using A = IntArith<GUARD>;
  __shared__ u64 lds[lds_words(LB)];
  const int j = blockIdx.x % nl;
  const size_t cc = blockIdx.x / nl;  // ct*2 + comp
  const size_t ct = cc >> 1;
  const int comp = (int)(cc & 1);
  const size_t N = (size_t)1 << LB;
  const Mod m = c.mods[j];
  const NttTable t = ntt_table(c, j);
  const u64 fix = round_fix(c.mods[c.K - 1].q >> 1, m);
  const DropInv d = inv_special_at(c, j);
  const u64 *__restrict__ src = tlast + cc * N;
  const u64 *__restrict__ ks = ksacc + (cc * nl + j) * N;
  u64 *__restrict__ o = out + (cc * nl + j) * N;
  if (addend && (comp == 0 || add_c1))  // workgroup-uniform: two straight-line bodies, no per-element select
    divround_finish<LB, A, false, true>(lds, m, t, fix, d, src, ks, addend + ct * addend_stride + ((size_t)comp * nl + j) * N, o);
  else
    divround_finish<LB, A, false, false>(lds, m, t, fix, d, src, ks, nullptr, o);
}

// K3, BFV: out[ct][comp][j] = (INTT_j(ksacc) - (tlast mod q_j + fix)) * q_sp^-1 (+ addend), coefficient form
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_moddown_bfv(DevCtx c, const u64 *__restrict__ ksacc,
                                                                         const u64 *__restrict__ tlast,
                                                                         const u64 *__restrict__ addend, size_t addend_stride,
                                                                         int add_c1, u64 *__restrict__ out, int nl) {
  __shared__ u64 lds[lds_words(LB)];
  const int j = blockIdx.x % nl;
  const size_t cc = blockIdx.x / nl;
  const size_t ct = cc >> 1;
  const int comp = (int)(cc & 1);
  const size_t N = (size_t)1 << LB;
  const Mod m = c.mods[j];
  const NttTable t = ntt_table(c, j);
  const u64 half = c.mods[c.K - 1].q >> 1;
  const u64 fix = round_fix(half, m);
  const u64 inv = c.cst->inv_special[j], inv_s = c.cst->inv_special_s[j];
  const u64 *__restrict__ src = tlast + cc * N;
  const u64 *__restrict__ ks = ksacc + (cc * nl + j) * N;
  u64 *__restrict__ o = out + (cc * nl + j) * N;
  auto ld = [&](int, int i) { return ks[i]; };
  if (addend && (comp == 0 || add_c1)) {
    const u64 *__restrict__ cin = addend + ct * addend_stride + ((size_t)comp * nl + j) * N;
    ntt_inv_block<LB>(
        lds, ld,
        [&](int, int i, u64 v) {
          const u64 x = add_mod(reduce64(src[i], m), fix, m.q);
          o[i] = add_mod(mul_shoup(sub_mod(scale_inv_n(v, m), x, m.q), inv, inv_s, m.q), cin[i], m.q);
        },
        t, m, 0, 0);
  } else {
    ntt_inv_block<LB>(
        lds, ld,
        [&](int, int i, u64 v) {
          const u64 x = add_mod(reduce64(src[i], m), fix, m.q);
          o[i] = mul_shoup(sub_mod(scale_inv_n(v, m), x, m.q), inv, inv_s, m.q);
        },
        t, m, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// fp64-only kernels (every key prime below 2^50: abc_ntt.hpp, "fp64 residue arithmetic"): the fused multiply front end
// and the split sequences
// ---------------------------------------------------------------------------------------------------------------
// four consecutive words as two adjacent 16-byte stores
__device__ __forceinline__ void store_run4(u64 *p, const u64 (&v)[4]) {
  reinterpret_cast<u64x2 *>(p)[0] = u64x2{v[0], v[1]};
  reinterpret_cast<u64x2 *>(p)[1] = u64x2{v[2], v[3]};
}
// |r| < q -> canonical u64
__device__ __forceinline__ u64 fp_small_to_canon(double r, double q) {
  const u32 neg = (u32)((int)(u32)((u64)__double_as_longlong(r) >> 32) >> 31);
  const u64 qb = (u64)__double_as_longlong(q);
  const u64 add = ((u64)((u32)(qb >> 32) & neg) << 32) | (u64)((u32)qb & neg);
  r += __longlong_as_double((long long)add);
  return (u64)__double_as_longlong(r + 4503599627370496.0) & 0x000fffffffffffffull;
}

// CKKS tensor product of one limb, as the load functor of the inverse transform of c2: element i of (a0,a1) x (b0,b1)
// -> c0, c1 and c2 (NTT form) to memory in whole 32-byte runs, c2 returned for the transform.  A lane owns runs of
// four consecutive words; writing the halves of a run far apart reached HBM as two partial-sector writes (PMC
// WRITE_SIZE 35 instead of 28 limbs per multiply), hence the staging of four values and the back-to-back stores.
struct TensorFront {
  const u64 *__restrict__ a0, *__restrict__ a1, *__restrict__ b0, *__restrict__ b1;
  u64 *__restrict__ o0, *__restrict__ o1, *__restrict__ dntt;
  double q, qinv;
  u64 t0[4], t1[4], t2[4];
  __device__ __forceinline__ TensorFront(const u64 *a, const u64 *b, u64 *c01, u64 *c2ntt, size_t ct, int j, int nl, size_t N,
                                         const Mod &m)
      : q(m.qd), qinv(m.qinv) {
    const size_t pw = (size_t)nl * N;
    a0 = a + ct * 2 * pw + j * N; a1 = a0 + pw;
    b0 = b + ct * 2 * pw + j * N; b1 = b0 + pw;
    o0 = c01 + ct * 2 * pw + j * N; o1 = o0 + pw;
    dntt = c2ntt + (ct * nl + j) * N;
  }
  __device__ __forceinline__ double operator()(int r, int i) {
    const double x0 = fp_from_u64(a0[i]), x1 = fp_from_u64(a1[i]), y0 = fp_from_u64(b0[i]), y1 = fp_from_u64(b1[i]);
    const double v = fp_mulmod(x1, y1, q, qinv);
    t0[r & 3] = fp_small_to_canon(fp_mulmod(x0, y0, q, qinv), q);
    t1[r & 3] = fp_to_canon(fp_mulmod(x0, y1, q, qinv) + fp_mulmod(x1, y0, q, qinv), q, qinv);
    t2[r & 3] = fp_small_to_canon(v, q);
    if ((r & 3) == 3) {
      store_run4(o0 + i - 3, t0);
      store_run4(o1 + i - 3, t1);
      store_run4(dntt + i - 3, t2);
    }
    return v;
  }
};

// fp64 twins of K2c and K3 (see "Where the twins stay" above K2c)
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_special_intt_fp(DevCtx c, const u64 *__restrict__ tsp,
                                                                             u64 *__restrict__ tlast) {
  __shared__ double lds[lds_words(LB)];
  const size_t N = (size_t)1 << LB;
  const Mod m = mod_at(c, c.K - 1);
  const FpTable t = fp_table(c, c.K - 1);
  const double half = (double)(m.q >> 1);
  const u64 *__restrict__ src = tsp + (size_t)blockIdx.x * N;
  u64 *__restrict__ dst = tlast + (size_t)blockIdx.x * N;
  ntt_inv_block_a<LB, FpArith>(
      lds, [&](int, int i) { return fp_from_u64(src[i]); },
      [&](int, int i, double v) { dst[i] = fp_to_canon(fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd) + half, m.qd, m.qinv); }, t, m, 0,
      0);
}

// K3, CKKS.  The special-prime polynomial (< q_sp <= 2^50) plus the rounding fix enters the transform unreduced
// (see K2a); the subtraction, the scaling by q_sp^-1 and the addend stay in doubles until the single
// canonicalisation of the store.
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_moddown_fp(DevCtx c, const u64 *__restrict__ ksacc,
                                                                        const u64 *__restrict__ tlast, const u64 *__restrict__ addend,
                                                                        size_t addend_stride, int add_c1, u64 *__restrict__ out, int nl,
                                                                        int ncc) {
  __shared__ double lds[lds_words(LB)];
  // The nl workgroups that read the same special-prime polynomial (ct, comp) are 8 apart in blockIdx: abc_context.hpp's xcd_slot,
  // spelt out here -- through the helper this kernel (alone of its callers) compiles to other register counts.
  const unsigned per = 8u * (unsigned)nl;
  const unsigned grp = blockIdx.x / per, rem = blockIdx.x % per;
  const unsigned left = (unsigned)ncc - grp * 8u, gsz = left < 8u ? left : 8u;  // the last group may be ragged
  const int j = (int)(rem / gsz);
  const size_t cc = (size_t)grp * 8 + rem % gsz;  // ct*2 + comp
  const size_t ct = cc >> 1;
  const int comp = (int)(cc & 1);
  const size_t N = (size_t)1 << LB;
  const Mod m = mod_at(c, j);
  const FpTable t = fp_table(c, j);
  const u64 half = c.mods[c.K - 1].q >> 1;
  const double fix = round_fix<double>(half, m);
  const double inv = c.cst->inv_special_c[j], inv_q = c.cst->inv_special_cq[j];
  const u64 *__restrict__ src = tlast + cc * N;
  const u64 *__restrict__ ks = ksacc + (cc * nl + j) * N;
  u64 *__restrict__ o = out + (cc * nl + j) * N;
  auto ld = [&](int, int i) { return fp_from_u64(src[i]) + fix; };
  if (addend && (comp == 0 || add_c1)) {  // workgroup-uniform: two straight-line bodies, no per-element select
    const u64 *__restrict__ cin = addend + ct * addend_stride + ((size_t)comp * nl + j) * N;
    ntt_fwd_block_a<LB, FpArith>(
        lds, ld,
        [&](int, int i, double v) {
          const double d = fp_from_u64(ks[i]) - v;
          o[i] = fp_to_canon(fp_mul_lazy(d, inv, inv_q, m.qd) + fp_from_u64(cin[(u32)i]), m.qd, m.qinv);
        },
        t, m, 0, 0);
  } else {
    ntt_fwd_block_a<LB, FpArith>(
        lds, ld,
        [&](int, int i, double v) {
          const double d = fp_from_u64(ks[i]) - v;
          o[i] = fp_to_canon(fp_mul_lazy(d, inv, inv_q, m.qd), m.qd, m.qinv);
        },
        t, m, 0, 0);
  }
}

// K3, BFV
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_ks_moddown_bfv_fp(DevCtx c, const u64 *__restrict__ ksacc,
                                                                            const u64 *__restrict__ tlast,
                                                                            const u64 *__restrict__ addend, size_t addend_stride,
                                                                            int add_c1, u64 *__restrict__ out, int nl) {
  __shared__ double lds[lds_words(LB)];
  const int j = blockIdx.x % nl;
  const size_t cc = blockIdx.x / nl;
  const size_t ct = cc >> 1;
  const int comp = (int)(cc & 1);
  const size_t N = (size_t)1 << LB;
  const Mod m = mod_at(c, j);
  const FpTable t = fp_table(c, j);
  const u64 half = c.mods[c.K - 1].q >> 1;
  const double fix = round_fix<double>(half, m);
  const double inv = c.cst->inv_special_c[j], inv_q = c.cst->inv_special_cq[j];
  const u64 *__restrict__ src = tlast + cc * N;
  const u64 *__restrict__ ks = ksacc + (cc * nl + j) * N;
  u64 *__restrict__ o = out + (cc * nl + j) * N;
  auto ld = [&](int, int i) { return fp_from_u64(ks[i]); };
  if (addend && (comp == 0 || add_c1)) {
    const u64 *__restrict__ cin = addend + ct * addend_stride + ((size_t)comp * nl + j) * N;
    ntt_inv_block_a<LB, FpArith>(
        lds, ld,
        [&](int, int i, double v) {
          const double d = fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd) - (fp_from_u64(src[i]) + fix);
          o[i] = fp_to_canon(fp_mul_lazy(d, inv, inv_q, m.qd) + fp_from_u64(cin[i]), m.qd, m.qinv);
        },
        t, m, 0, 0);
  } else {
    ntt_inv_block_a<LB, FpArith>(
        lds, ld,
        [&](int, int i, double v) {
          const double d = fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd) - (fp_from_u64(src[i]) + fix);
          o[i] = fp_to_canon(fp_mul_lazy(d, inv, inv_q, m.qd), m.qd, m.qinv);
        },
        t, m, 0, 0);
  }
}

// K1 + K2a in one workgroup (CKKS multiply): the coefficients of c2_j leave the inverse transform in exactly the
// register layout the forward transform's first pass loads (PassIdx<LB,0,R0> both ways), so they stay in 16
// registers per lane and feed the nl forward transforms modulo the other key primes back to back -- the
// coefficient form of c2 never touches HBM (saves 4 + 16 limb transfers per ciphertext and one launch).
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_tensor_decomp_fp(DevCtx c, const u64 *__restrict__ a,
                                                                           const u64 *__restrict__ b, u64 *__restrict__ c01,
                                                                           u64 *__restrict__ c2ntt, u64 *__restrict__ dec, int nl) {
  __shared__ double lds[lds_words(LB)];
  const int j = blockIdx.x % nl;
  const size_t ct = blockIdx.x / nl;
  const size_t N = (size_t)1 << LB;
  double src[16];
  {
    const Mod m = mod_at(c, j);
    const FpTable t = fp_table(c, j);
    TensorFront front(a, b, c01, c2ntt, ct, j, nl, N, m);
    ntt_inv_block_a<LB, FpArith>(
        lds, [&](int r, int i) { return front(r, i); },
        // canonical [0, q_j) as a double: the value SEAL's decomposition reduces modulo the other primes
        [&](int r, int, double v) {
          const double w = fp_centre(fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd), m.qd, m.qinv);
          src[r] = w < 0.0 ? w + m.qd : w;
        },
        t, m, 0, 0);
  }
  for (int I = 0; I <= nl; I++) {
    if (I == j) continue;
    const int ki = (I == nl) ? c.K - 1 : I;
    const Mod m = mod_at(c, ki);
    const FpTable t = fp_table(c, ki);
    u64 *__restrict__ dst = dec + ((ct * (nl + 1) + I) * nl + j) * N;
    block_sync_lds();  // the previous transform's last pass has read its LDS words
    ntt_fwd_block_a<LB, FpArith>(
        lds, [&](int r, int) { return src[r]; }, [&](int, int i, double v) { dst[i] = fp_to_lazy(v, m.qd, m.qinv); }, t, m, 0, 0);
  }
}

// the sixteen stride-2^(LB-4) values of a lane after the first register pass of a forward transform -> the half-done limb at dst,
// raw doubles (kind 0) or centred and packed (abc_ntt.hpp, "packed half-done limbs"); kind is workgroup-uniform
template <int LB>
__device__ __forceinline__ void store_half_done(double *__restrict__ dst, double (&y)[16], int p, const FpK &kk, int kind) {
  constexpr size_t N = (size_t)1 << LB;
  constexpr int SH = LB - 4;
  if (kind == 0) {
#pragma unroll
    for (int k = 0; k < 16; k++) dst[(k << SH) + p] = y[k];
  } else if (kind == 1) {
#pragma unroll
    for (int k = 0; k < 16; k++) pack_store<1>(dst, N, (size_t)(k << SH) + p, fp_centre(y[k], kk.q, kk.qinv));
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) pack_store<2>(dst, N, (size_t)(k << SH) + p, fp_centre(y[k], kk.q, kk.qinv));
  }
}

// ---- split transforms (N = 2^14) ------------------------------------------------------------------------------------
// A 2^14-point forward transform is a radix-16 pass over stride-1024 elements (stages 0..3, no LDS: the sixteen
// operands of a lane are exactly what the inverse transform's last pass leaves in its registers) followed by
// sixteen independent 1024-point transforms (stages 4..13) that one wavefront each completes in 8.5 KiB of LDS.
// The first kernel of a sequence does the LDS-resident part (tensor product or operand, inverse transform of limb j) and the
// register pass of the forward transforms, and stores the half-done limbs (raw doubles or packed, abc_ntt.hpp); the later
// kernels finish them block by block and multiply into the key on the fly.

// K1s for a general key switch.  CKKS (the operand arrives in NTT form): inverse transform of limb j in LDS, then the
// register pass modulo every other key prime.  BFV (coefficient form): no LDS at all, the register pass modulo every key
// prime including q_j itself.
template <int LB, bool CKKS, bool GAL>
__global__ __launch_bounds__((1 << LB) / 16) void k_fused_operand_pass0_fp(DevCtx c, const u64 *__restrict__ src, size_t src_stride,
                                                                           double *__restrict__ part, int nl, int per_target,
                                                                           u32 gelt, int padded) {
  static_assert(LB == 14, "split transforms are laid out for N = 2^14");
  __shared__ double lds[CKKS ? lds_words(LB) : 1];
  const size_t N = (size_t)1 << LB;
  // per_target (BFV, few ciphertexts in flight): one workgroup per (ct, J, target I) instead of per (ct, J), so a
  // single-ciphertext call spreads over nl (nl+1) CUs rather than nl
  const unsigned wg = per_target ? blockIdx.x / (unsigned)(nl + 1) : blockIdx.x;
  const int only = per_target ? (int)(blockIdx.x % (unsigned)(nl + 1)) : -1;
  const int j = wg % nl;
  const size_t ct = wg / nl;
  const int tid = threadIdx.x;
  const u64 *__restrict__ sp = src + ct * src_stride + (size_t)j * N;
  double x[16];
  if constexpr (CKKS) {
    const Mod m = mod_at(c, j);
    const FpTable t = fp_table(c, j);
    ntt_inv_block_a<LB, FpArith>(
        lds, [&](int, int i) { return fp_from_u64(sp[galois_ntt_src<GAL>((u32)i, gelt, LB)]); },  // gelt: rotation folded in
        [&](int r, int, double v) {
          double w = fp_centre(fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd), m.qd, m.qinv);
          x[r] = w < 0.0 ? w + m.qd : w;
        },
        t, m, 0, 0);
  } else if (gelt) {  // BFV rotation: gelt = elt^-1 mod 2N, the permutation (with its sign) folded into the load -- workgroup-uniform
    const u64 qj = c.mods[j].q;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      bool neg;
      const u64 v = sp[galois_coef_src((u32)((k << 10) + tid), gelt, LB, neg)];
      x[k] = fp_from_u64(neg ? neg_mod(v, qj) : v);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = fp_from_u64(sp[(k << 10) + tid]);
  }
  const int hi0[1] = {0};
  for (int I = 0; I <= nl; I++) {
    if (CKKS && I == j) continue;
    if (only >= 0 && I != only) continue;
    const int ki = (I == nl) ? c.K - 1 : I;
    const Mod m = mod_at(c, ki);
    const FpTable t = fp_table(c, ki);
    const FpK kk = FpArith::consts(m);
    double y[16];
#pragma unroll
    for (int k = 0; k < 16; k++) y[k] = x[k];
    fwd_pass<FpArith, LB, 0, 4>(y, hi0, t, kk, 0, 0);
    double *__restrict__ dst = part + ((ct * (nl + 1) + I) * nl + j) * ((padded & 1) ? (size_t)c.ps : N);
    store_half_done<LB>(dst, y, tid, kk, ((padded & 2) && I < nl) ? pack_kind(m.bits) : 0);  // padded bit 1: packed (data primes only)
  }
}

// ---- the split sequence of the hot call (N = 2^14, CKKS, every key prime < 2^50): four launches, 84 limb transfers -----------
//   K1  k_split2_tensor_pass0_fp (multiply) / k_fused_operand_pass0_fp (rotation, relinearise): reads only a1, b1 (c2 = a1 b1 is
//       all the key switch needs), inverse transform in LDS, register pass modulo every other key prime -> half-done limbs
//   K2a k_split_special_fp: the special prime's inner product and the block-local part of its inverse transform
//   K2b k_split3_pass_fp (registers only): last radix-16 pass of that inverse transform, N^-1, + q_sp/2, then for every data prime
//       q_j the first radix-16 pass of the forward transform of (t mod q_j): half-done mod-down limbs
//   K2c k_split4_main_fp (up to five data limbs) / k_split3_main_fp, per (ct, data prime I, block): nl - 1 wavefronts finish the
//       decomposition limbs, two more the mod-down limbs of K2b on the same block, then every thread forms, for two adjacent
//       coefficients,   out_c = (sum_J x_J key_J,c + q_sp c_c - NTT_I(t_c)) q_sp^-1   (mod q_I)
//       with the diagonal operand c2_I = a1 b1 and c0 = a0 b0, c1 = a0 b1 + a1 b0 computed right there from a and b and folded in
//       as q_sp c:  (acc + q_sp c - NTT(t)) q_sp^-1 = (acc - NTT(t)) q_sp^-1 + c.  Neither c0, c1 nor c2's NTT form ever travel
//       through scratch, the accumulators never leave the CU, sums over J are formed in registers (no LDS atomics), and `out`
//       may alias an operand (a and b are last read here, by the thread that then writes those words).
// (Earlier generations -- LDS-atomic tail kernels, the LDS-resident mod-down, an LDS-table twin of K2a -- were measured in
// rounds 1 and 2 and are gone: DESIGN.md section 4.)
template <int LB>
__global__ __launch_bounds__((1 << LB) / 16) void k_split2_tensor_pass0_fp(DevCtx c, const u64 *__restrict__ a,
                                                                           const u64 *__restrict__ b, double *__restrict__ part,
                                                                           int nl, int pack) {
  static_assert(LB == 14, "split transforms are laid out for N = 2^14");
  __shared__ double lds[lds_words(LB)];
  const int j = blockIdx.x % nl;
  const size_t ct = blockIdx.x / nl;
  const size_t N = (size_t)1 << LB, pw = (size_t)nl * N;
  double src[16];
  {
    const Mod m = mod_at(c, j);
    const FpTable t = fp_table(c, j);
    const u64 *__restrict__ a1 = a + ct * 2 * pw + pw + (size_t)j * N, *__restrict__ b1 = b + ct * 2 * pw + pw + (size_t)j * N;
    const double q = m.qd, qinv = m.qinv;
    ntt_inv_block_a<LB, FpArith>(
        lds, [&](int, int i) { return fp_mulmod(fp_from_u64(a1[i]), fp_from_u64(b1[i]), q, qinv); },
        // canonical [0, q_j) as a double: the value SEAL's decomposition reduces modulo the other primes
        [&](int r, int, double v) {
          const double w = fp_centre(fp_mul_lazy(v, m.inv_n_c, m.inv_n_cq, m.qd), m.qd, m.qinv);
          src[r] = w < 0.0 ? w + m.qd : w;
        },
        t, m, 0, 0);
  }
  const int tid = threadIdx.x;
  const int hi0[1] = {0};
  for (int I = 0; I <= nl; I++) {
    if (I == j) continue;
    const int ki = (I == nl) ? c.K - 1 : I;
    const Mod m = mod_at(c, ki);
    const FpTable t = fp_table(c, ki);
    const FpK kk = FpArith::consts(m);
    double y[16];
#pragma unroll
    for (int k = 0; k < 16; k++) y[k] = src[k];
    fwd_pass<FpArith, LB, 0, 4>(y, hi0, t, kk, 0, 0);
    double *__restrict__ dst = part + ((ct * (nl + 1) + I) * nl + j) * (size_t)c.ps;
    store_half_done<LB>(dst, y, tid, kk, (pack && I < nl) ? pack_kind(m.bits) : 0);  // the special prime's limbs stay raw
  }
}

// K2a, the special prime's share of the key inner product (grid (ct, block); nl wavefronts): wavefront J finishes stages 4..13 of
// the half-done limb (ct, special prime, J) on this 1024-point block and parks it in LDS; after one barrier every thread sums, for
// two adjacent coefficients, x_J key[J][c][special] over J in registers; the two sums go back to LDS and wavefronts 0 and 1 run
// the ten block-local stages of the special-prime limb's INVERSE transform on them -> tsp_half (raw doubles); k_split3_pass_fp
// does the remaining radix-16 pass.  NL > 0: compile-time limb count (the loop over J unrolls, all its loads are issued
// together); NL = 0: any nl <= 12.
template <int NL>
__global__ __launch_bounds__(NL ? NL * 64 : 768) void k_split_special_fp(DevCtx c, const double *__restrict__ part, const u64 *__restrict__ key,
                                                                         const double *__restrict__ keyf, double *__restrict__ tsp_half,
                                                                         int nl_rt) {
  extern __shared__ double dyn[];  // max(nl, 2) buffers of one 1024-point block each
  const int nl = NL ? NL : nl_rt;
  const int J = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x & 15;
  const size_t ct = (size_t)(blockIdx.x >> 4);
  const size_t N = (size_t)c.n, base = (size_t)blk << 10;
  const int ki = c.K - 1;
  const Mod m = mod_at(c, ki);
  const FpTable t = fp_table(c, ki);
  const double q = m.qd, qinv = m.qinv;
  {
    double *buf = dyn + J * lds_words(10);
    const double *__restrict__ src = part + ((ct * (nl + 1) + nl) * nl + J) * (size_t)c.ps + base;
    ntt_fwd_block_a<10, FpTail>(
        buf, [&](int, int i) { return fp_centre(src[i], q, qinv); }, [&](int, int i, double v) { buf[lds_pad(i)] = v; }, t, m, 4, blk,
        lane);
  }
  __syncthreads();
  for (int e = 2 * (int)threadIdx.x; e < 1024; e += 2 * (int)blockDim.x) {  // this thread: coefficients e, e + 1 of the block
    double s0[2] = {0.0, 0.0}, s1[2] = {0.0, 0.0};
#pragma unroll
    for (int Jx = 0; Jx < (NL ? NL : 12); Jx++) {
      if (!NL && Jx >= nl) break;
      const f64x2 v = *reinterpret_cast<const f64x2 *>(dyn + Jx * lds_words(10) + lds_pad(e));
      const size_t i0 = (((size_t)Jx * 2 + 0) * c.K + ki) * N + base + e, i1 = i0 + (size_t)c.K * N;
      f64x2 k0, k1;
      if (keyf) {  // the key's fp64 twin (workgroup-uniform): no conversion
        k0 = *reinterpret_cast<const f64x2 *>(keyf + i0);
        k1 = *reinterpret_cast<const f64x2 *>(keyf + i1);
      } else {
        const u64x2 r0 = *reinterpret_cast<const u64x2 *>(key + i0), r1 = *reinterpret_cast<const u64x2 *>(key + i1);
        k0.x = fp_from_u64(r0.x); k0.y = fp_from_u64(r0.y);
        k1.x = fp_from_u64(r1.x); k1.y = fp_from_u64(r1.y);
      }
      s0[0] += fp_mulmod(v.x, k0.x, q, qinv);
      s0[1] += fp_mulmod(v.y, k0.y, q, qinv);
      s1[0] += fp_mulmod(v.x, k1.x, q, qinv);
      s1[1] += fp_mulmod(v.y, k1.y, q, qinv);
      if (Jx == 7) {  // eight products of magnitude < q stay below 2^53; re-centre before adding more
#pragma unroll
        for (int k = 0; k < 2; k++) {
          s0[k] = fp_centre(s0[k], q, qinv);
          s1[k] = fp_centre(s1[k], q, qinv);
        }
      }
    }
    // park the two sums (centred) in buffers 0 and 1; this thread has read its words of them already
    f64x2 r;
    r.x = fp_centre(s0[0], q, qinv); r.y = fp_centre(s0[1], q, qinv);
    *reinterpret_cast<f64x2 *>(dyn + lds_pad(e)) = r;
    r.x = fp_centre(s1[0], q, qinv); r.y = fp_centre(s1[1], q, qinv);
    *reinterpret_cast<f64x2 *>(dyn + lds_words(10) + lds_pad(e)) = r;
  }
  __syncthreads();
  for (int comp = J; comp < 2; comp += nl) {  // one wavefront per component
    double *buf = dyn + comp * lds_words(10);
    double *__restrict__ dst = tsp_half + (ct * 2 + comp) * (size_t)c.ps + base;
    ntt_inv_block_a<10, FpArith>(
        buf, [&](int, int i) { return buf[lds_pad(i)]; }, [&](int, int i, double v) { dst[i] = v; }, t, m, 4, blk, lane);
  }
}

static void launch_split_special(hipStream_t st, abc_hip_ctx *c, size_t cc, int nl, const double *part, const u64 *key, double *tsp_half) {
  const dim3 grid((unsigned)(cc * 16)), block(64 * nl);
  const size_t lds = (size_t)((nl < 2 ? 2 : nl) * lds_words(10)) * 8;
  const double *keyf = key_twin_lookup(c, key);
#define ABC_SP(NLV) hipLaunchKernelGGL((k_split_special_fp<NLV>), grid, block, lds, st, c->dc, part, key, keyf, tsp_half, nl)
  switch (nl) {
    case 1: ABC_SP(1); break;
    case 2: ABC_SP(2); break;
    case 3: ABC_SP(3); break;
    case 4: ABC_SP(4); break;
    default: ABC_SP(0); break;
  }
#undef ABC_SP
}

// fused_scratch_limbs(L) (abc_route.hpp) per ciphertext: coef L, ntt L, dec L(L+1), ksacc 2L, tsp 2, tlast 2, c01 2L
struct FusedScratch {
  u64 *coef, *ntt, *dec, *ksacc, *tsp, *tlast, *c01;
};
static inline FusedScratch carve(u64 *base, size_t chunk, int nl, size_t N) {
  FusedScratch s;
  s.coef = base;
  s.ntt = s.coef + chunk * nl * N;
  s.dec = s.ntt + chunk * nl * N;
  s.ksacc = s.dec + chunk * nl * (nl + 1) * N;
  s.tsp = s.ksacc + chunk * 2 * nl * N;
  s.tlast = s.tsp + chunk * 2 * N;
  s.c01 = s.tlast + chunk * 2 * N;
  return s;
}


template <int LB>
__global__ __launch_bounds__(256) void k_split3_pass_fp(DevCtx c, const double *__restrict__ tsp_half, double *__restrict__ tpart, int nl,
                                                        int pack) {
  static_assert(LB == 14, "split transforms are laid out for N = 2^14");
  const size_t cc = blockIdx.x >> 2;                                  // ct*2 + comp
  const int p = (int)((blockIdx.x & 3) << 8) + (int)threadIdx.x;      // position inside every 1024-point block
  const int hi0[1] = {0};
  double x[16];
  {
    const Mod ms = mod_at(c, c.K - 1);
    const FpTable ts = fp_table(c, c.K - 1);
    const FpK ks = FpArith::consts(ms);
    const double *__restrict__ src = tsp_half + cc * (size_t)c.ps;
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = src[(k << 10) + p];
    FpArith::centre16(x, ks);
    inv_pass<FpArith, LB, 0, 4>(x, hi0, ts, ks, 0, 0);
    const double half = (double)(ms.q >> 1);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const double w = fp_centre(fp_mul_lazy(x[k], ms.inv_n_c, ms.inv_n_cq, ms.qd) + half, ms.qd, ms.qinv);
      x[k] = w < 0.0 ? w + ms.qd : w;  // canonical [0, q_sp): what SEAL reduces modulo q_j
    }
  }
  const u64 half = c.mods[c.K - 1].q >> 1;
  for (int j = 0; j < nl; j++) {
    const Mod m = mod_at(c, j);
    const FpTable t = fp_table(c, j);
    const FpK kk = FpArith::consts(m);
    const double fix = round_fix<double>(half, m);
    double y[16];
#pragma unroll
    for (int k = 0; k < 16; k++) y[k] = x[k] + fix;
    fwd_pass<FpArith, LB, 0, 4>(y, hi0, t, kk, 0, 0);
    double *__restrict__ dst = tpart + (cc * nl + j) * (size_t)c.ps;
    store_half_done<LB>(dst, y, p, kk, pack ? pack_kind(m.bits) : 0);
  }
}

// A = WithAcc (MODE 1, one more argument): a second, ungathered ciphertext `acc` [ct][2][nl][N] is added, read at the thread's own
// index (rotate_add: out = acc + rotate(in)).  `out` may be `acc`: a thread loads its two coefficients of either component before
// it stores them.  Without it the pack is empty and the kernel is, name and code, the one it was.
// A = WithMac (MODE 1, rotate_mac_plain): out = acc + plain (.) rotate(in).  The plaintext multiplies the finished, centred pair of
// either component -- |r| <= q/2 times a canonical word, |product| < q -- and the canonical acc word joins it: below 2q, which
// fp_to_canon centres exactly.  The rotation's own c0 stays in d0 (it is multiplied too), so acc cannot be pre-added there.  All
// three pairs are loaded ahead of the thread's stores: `out` may be `acc`.  A null acc is a workgroup-uniform branch.
template <int MODE, bool GAL, int NL, class... A>
__global__ __launch_bounds__(NL ? (NL + 1) * 64 : 832) void k_split3_main_fp(DevCtx c, const double *__restrict__ part,
                                                                              const double *__restrict__ tpart,
                                                                              const u64 *__restrict__ opa, const u64 *__restrict__ opb,
                                                                              size_t opa_stride, size_t opb_stride, int add_c1,
                                                                              const u64 *__restrict__ key, u64 *__restrict__ out, int nl_rt,
                                                                              u32 gelt, AccArg<A>... acc_) {
  constexpr bool ACC = kWithAcc<A...>, MAC = kWithMac<A...>;
  static_assert(!(ACC || MAC) || MODE == 1, "the second addend belongs to the key switch");
  [[maybe_unused]] const u64 *acc = acc_ptr(acc_...);
  [[maybe_unused]] const AccArg<WithMac> mac = mac_arg(acc_...);
  extern __shared__ double dyn[];  // nl + 1 buffers of one 1024-point block: nl - 1 decomposition limbs, 2 mod-down limbs
  const int nl = NL ? NL : nl_rt;
  const int W = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x & 15;
  const int I = (int)((blockIdx.x >> 4) % nl);
  const size_t ct = (size_t)((blockIdx.x >> 4) / nl);
  const size_t N = (size_t)c.n, base = (size_t)blk << 10;
  const Mod m = mod_at(c, I);
  const FpTable t = fp_table(c, I);
  const double q = m.qd, qinv = m.qinv;
  {
    double *buf = dyn + W * lds_words(10);
    const double *__restrict__ src;
    if (W < nl - 1) {
      const int J = W < I ? W : W + 1;
      src = part + ((ct * (nl + 1) + I) * nl + J) * (size_t)c.ps + base;
    } else {
      src = tpart + ((ct * 2 + (W - (nl - 1))) * nl + I) * (size_t)c.ps + base;
    }
    ntt_fwd_block_a<10, FpArith>(
        buf, [&](int, int i) { return fp_centre(src[i], q, qinv); }, [&](int, int i, double v) { buf[lds_pad(i)] = v; }, t, m, 4, blk,
        lane);
  }
  __syncthreads();
  const double inv = c.cst->inv_special_c[I], inv_q = c.cst->inv_special_cq[I];
  const size_t pw = (size_t)nl * N;
  const double *tt0 = dyn + (nl - 1) * lds_words(10), *tt1 = dyn + nl * lds_words(10);
  for (int e = 2 * (int)threadIdx.x; e < 1024; e += 2 * (int)blockDim.x) {  // this thread: coefficients e, e + 1 of the block
    double s0[2] = {0.0, 0.0}, s1[2] = {0.0, 0.0}, d0[2] = {0.0, 0.0}, d1[2] = {0.0, 0.0};
    [[maybe_unused]] u64x2 mp = {0, 0}, ma0 = {0, 0}, ma1 = {0, 0};
    if constexpr (MAC) {  // the thread's own pair of the plaintext and of either component of acc, ahead of the stores
      mp = *reinterpret_cast<const u64x2 *>(mac.plain + ct * mac.plain_stride + (size_t)I * N + base + e);
      if (acc) {
        const u64 *ac = acc + ct * 2 * pw + (size_t)I * N + base + e;
        ma0 = *reinterpret_cast<const u64x2 *>(ac);
        ma1 = *reinterpret_cast<const u64x2 *>(ac + pw);
      }
    }
#pragma unroll
    for (int Jx = 0; Jx < (NL ? NL : 12); Jx++) {
      if (!NL && Jx >= nl) break;
      double x[2];
      if (Jx == I) {
        if (MODE == 0) {
          const u64 *pa = opa + ct * 2 * pw + (size_t)I * N + base + e, *pb = opb + ct * 2 * pw + (size_t)I * N + base + e;
          const u64x2 a0 = *reinterpret_cast<const u64x2 *>(pa), a1 = *reinterpret_cast<const u64x2 *>(pa + pw);
          const u64x2 b0 = *reinterpret_cast<const u64x2 *>(pb), b1 = *reinterpret_cast<const u64x2 *>(pb + pw);
          const double x0[2] = {fp_from_u64(a0.x), fp_from_u64(a0.y)}, x1[2] = {fp_from_u64(a1.x), fp_from_u64(a1.y)};
          const double y0[2] = {fp_from_u64(b0.x), fp_from_u64(b0.y)}, y1[2] = {fp_from_u64(b1.x), fp_from_u64(b1.y)};
#pragma unroll
          for (int k = 0; k < 2; k++) {
            x[k] = fp_mulmod(x1[k], y1[k], q, qinv);
            d0[k] = fp_mulmod(x0[k], y0[k], q, qinv);
            d1[k] = fp_mulmod(x0[k], y1[k], q, qinv) + fp_mulmod(x1[k], y0[k], q, qinv);
          }
        } else {
          const u64 *xl = opa + ct * opa_stride + (size_t)I * N;  // whole limb: a rotation gathers across blocks
#pragma unroll
          for (int k = 0; k < 2; k++) {
            const u32 si = galois_ntt_src<GAL>((u32)(base + e + k), gelt, c.logn);
            x[k] = fp_from_u64(xl[si]);
            if (opb) {
              const u64 *ad = opb + ct * opb_stride + (size_t)I * N;
              if constexpr (ACC) {
                // two canonical residues added as integers: below 2q <= 2^51, so the conversion stays exact; behind
                // fp_mul_lazy (|.| <= q) fp_to_canon then sees less than 3q < 2^52 and still centres exactly
                const u64 *ac = acc + ct * 2 * pw + (size_t)I * N + base + e + k;
                d0[k] = fp_from_u64(ad[si] + ac[0]);
                d1[k] = fp_from_u64(add_c1 ? ad[pw + si] + ac[pw] : ac[pw]);
              } else {
                d0[k] = fp_from_u64(ad[si]);
                if (add_c1) d1[k] = fp_from_u64(ad[pw + si]);
              }
            }
          }
        }
      } else {
        const int w = Jx < I ? Jx : Jx - 1;
        const f64x2 v = *reinterpret_cast<const f64x2 *>(dyn + w * lds_words(10) + lds_pad(e));
        x[0] = v.x;
        x[1] = v.y;
      }
      const u64x2 k0 = *reinterpret_cast<const u64x2 *>(key + (((size_t)Jx * 2 + 0) * c.K + I) * N + base + e);
      const u64x2 k1 = *reinterpret_cast<const u64x2 *>(key + (((size_t)Jx * 2 + 1) * c.K + I) * N + base + e);
      s0[0] += fp_mulmod(x[0], fp_from_u64(k0.x), q, qinv);
      s0[1] += fp_mulmod(x[1], fp_from_u64(k0.y), q, qinv);
      s1[0] += fp_mulmod(x[0], fp_from_u64(k1.x), q, qinv);
      s1[1] += fp_mulmod(x[1], fp_from_u64(k1.y), q, qinv);
      if (Jx == 7) {  // eight products of magnitude < q stay below 2^53; re-centre before adding more
#pragma unroll
        for (int k = 0; k < 2; k++) {
          s0[k] = fp_centre(s0[k], q, qinv);
          s1[k] = fp_centre(s1[k], q, qinv);
        }
      }
    }
    const f64x2 u0 = *reinterpret_cast<const f64x2 *>(tt0 + lds_pad(e)), u1 = *reinterpret_cast<const f64x2 *>(tt1 + lds_pad(e));
    // (sum + q_sp (c0, c1) - NTT(t)) q_sp^-1
    u64x2 r;
    if constexpr (MAC) {
      const double p0 = fp_from_u64(mp.x), p1 = fp_from_u64(mp.y);
      r.x = fp_mac_canon(fp_mul_lazy(s0[0] - u0.x, inv, inv_q, q) + d0[0], p0, ma0.x, q, qinv);
      r.y = fp_mac_canon(fp_mul_lazy(s0[1] - u0.y, inv, inv_q, q) + d0[1], p1, ma0.y, q, qinv);
      *reinterpret_cast<u64x2 *>(out + ((ct * 2 + 0) * nl + I) * N + base + e) = r;
      r.x = fp_mac_canon(fp_mul_lazy(s1[0] - u1.x, inv, inv_q, q) + d1[0], p0, ma1.x, q, qinv);
      r.y = fp_mac_canon(fp_mul_lazy(s1[1] - u1.y, inv, inv_q, q) + d1[1], p1, ma1.y, q, qinv);
      *reinterpret_cast<u64x2 *>(out + ((ct * 2 + 1) * nl + I) * N + base + e) = r;
      continue;
    }
    r.x = fp_to_canon(fp_mul_lazy(s0[0] - u0.x, inv, inv_q, q) + d0[0], q, qinv);
    r.y = fp_to_canon(fp_mul_lazy(s0[1] - u0.y, inv, inv_q, q) + d0[1], q, qinv);
    *reinterpret_cast<u64x2 *>(out + ((ct * 2 + 0) * nl + I) * N + base + e) = r;
    r.x = fp_to_canon(fp_mul_lazy(s1[0] - u1.x, inv, inv_q, q) + d1[0], q, qinv);
    r.y = fp_to_canon(fp_mul_lazy(s1[1] - u1.y, inv, inv_q, q) + d1[1], q, qinv);
    *reinterpret_cast<u64x2 *>(out + ((ct * 2 + 1) * nl + I) * N + base + e) = r;
  }
}

template <int MODE, bool GAL>
static void launch_split3_main(abc_hip_ctx *c, const MainArgs &a) {
  const KsOperands &o = a.ops;
  const int nl = o.nl;
  const dim3 grid((unsigned)(o.count * nl * 16)), block(64 * (nl + 1));
  const size_t lds = (size_t)((nl + 1) * lds_words(10)) * 8;
  dispatch_nl<0, 4>(nl <= 4 ? nl : 0, [&](auto NL) {  // 0: the form with a run-time limb count
    dispatch_tail<MODE == 1 && GAL, MODE == 1 && GAL>(o, [&](auto... tail) {
      hipLaunchKernelGGL((k_split3_main_fp<MODE, GAL, decltype(NL)::value, typename decltype(tail)::tag...>), grid, block, lds, a.st, c->dc,
                         (const double *)a.part, (const double *)a.tpart, o.target, o.addend, o.target_stride, o.addend_stride, o.add_c1, o.key,
                         o.out, nl, o.gather, tail...);
    });
  });
}


// ---- "split4": K2c with every vector-memory request issued up front ----------------------------------------------------------
// Same arithmetic and the same buffers as k_split3_main_fp.  What changes is the order of memory requests inside a wavefront:
// the per-lane twiddles of the tail transform come from an LDS table of the block's own twiddles (8 KiB per workgroup, filled
// cooperatively) instead of vector loads, so nothing in the transform touches the in-order vector-memory counter any more and
// the operands of the phase AFTER the transform (key slices, a and b) can be requested before it: one exposed memory latency per
// workgroup instead of two, and the transform runs under the second one.
// HALVES (nl <= 4): the pair phase one output component at a time.  The key words of one component share one register set, the
// non-diagonal digits are read from LDS once per half, and every operand of the pair phase is requested after this wavefront's
// transform instead of before it: 70 VGPRs, so that three workgroups fit a CU by registers as well as by LDS (3 x 50.5 KiB).
// Without it the pair phase is in one piece with its operands prefetched across the transform (nl = 5..7, where LDS allows two
// workgroups per CU anyway, and ABC_HIP_MAIN_TWO_PER_CU=1).  The sums, their order and every rounding are the same: same bits.
template <int MODE, int NL, bool HALVES>
struct PairOps {
  u64x2 k[HALVES ? NL : 2 * NL];  // HALVES: digit Jx of the component in hand; otherwise [2 Jx + component]
  u64x2 a0, a1, b0, b1;           // MODE 0
  u64 xs[2], d0s[2], d1s[2];      // MODE 1
};

// A = WithAcc (MODE 1, one more argument): the second, ungathered ciphertext of rotate_add, as in k_split3_main_fp.  Its words are
// added to the gathered addend as integers when the operands are loaded -- d0s < 2q <= 2^51, d1s < q (2q with add_c1) -- so PairOps
// holds what it held, and both forms still load every operand before their first store.
// A = WithMac (MODE 1, rotate_mac_plain): out = acc + plain (.) rotate(in), as in k_split3_main_fp: `finish` multiplies the centred
// pair by the thread's own plaintext pair and adds acc's.  d0s keeps the rotation's own c0 alone: the plaintext multiplies it too.
template <int MODE, bool GAL, int NL, bool HALVES, class... A>
__global__ __launch_bounds__(512, HALVES ? 6 : NL <= 4 ? 4 : 2) void k_split4_main_fp(DevCtx c, const double *__restrict__ part,
                                                                   const double *__restrict__ tpart, const u64 *__restrict__ opa,
                                                                   const u64 *__restrict__ opb, size_t opa_stride, size_t opb_stride,
                                                                   int add_c1, const u64 *__restrict__ key, u64 *__restrict__ out, u32 gelt,
                                                                   u32 imap, int ni, int pack, const double *__restrict__ keyf,
                                                                   AccArg<A>... acc_) {
  constexpr bool ACC = kWithAcc<A...>, MAC = kWithMac<A...>;
  static_assert(!(ACC || MAC) || MODE == 1, "the second addend belongs to the key switch");
  [[maybe_unused]] const u64 *acc = acc_ptr(acc_...);
  [[maybe_unused]] const AccArg<WithMac> mac = mac_arg(acc_...);
  // grid (ct, slot, block), slot < ni; the data prime of a slot is nibble `slot` of imap (all of them: 0x76543210, ni = nl; a subset
  // when a chain mixes fp64-capable and wider primes: abc_kernels_isplit.hip)
  // pack: the half-done limbs of `part` / `tpart` modulo primes of at most 48 bits arrive packed (abc_ntt.hpp)
  extern __shared__ double dyn[];  // nl + 1 transform buffers, then the block's twiddle table (1024 doubles)
  // 512 threads whatever nl: one coefficient pair per thread afterwards, so every operand of that phase is requested up front;
  // wavefronts nl + 1 .. 7 have no limb to transform and only take part in the table fill and the inner product
  static_assert(NL + 1 <= 8, "one wavefront per limb, eight wavefronts");
  static_assert(!HALVES || NL <= 4, "three workgroups per CU: four transform buffers at the most");
  constexpr int nl = NL, NT = 512, PER = 2;
  // LATE: digits whose key words are requested AFTER the transform.  The multiply at four limbs holds 48 VGPRs of prefetched
  // operands across the transform and sits on the 128-VGPR ceiling of two workgroups per CU; the butterfly's quotient now hangs
  // on its own product (one multiply more in the chain, abc_ntt.hpp), which cost five more live registers and, with everything
  // prefetched, 20 bytes of scratch per lane -- scratch reloads go through the same in-order vmcnt as the prefetch.  The last
  // digit's eight registers are therefore loaded late: its words come out of L2 and are used last, behind the other digits'
  // products (123 VGPRs, no scratch).  HALVES requests everything late.
  // (the second addend's two loads put the one-piece key switch at four limbs in the same place: 36 bytes of scratch without it)
  constexpr int LATE = (!HALVES && (MODE == 0 || ACC || MAC) && NL == 4) ? 1 : 0;
  // MAC_LATE: up to four limbs the one-piece form (128 VGPRs for four workgroups per CU) requests the plaintext and acc pairs
  // after the transform as well: ahead of it they cost 12 to 16 bytes of scratch at three and four limbs
  constexpr bool MAC_LATE = !HALVES && MAC && NL <= 4;
  // MAC_INNER: HALVES at four limbs sits at 70 of its 80 VGPRs; there each half requests its pairs behind its sum, when the key
  // words are dead: 80 VGPRs, no scratch (with the operands: 80 and 28 bytes of scratch).  Measured against the one-piece form
  // (117 VGPRs, two workgroups per CU) at batch 512: 1.18 - 1.22 ms against 1.25 - 1.28 per call, so HALVES stays
  constexpr bool MAC_INNER = HALVES && MAC && NL == 4;
  using Ops = PairOps<MODE, NL, HALVES>;
  const int W = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x & 15;
  const int I = (int)((imap >> (4 * ((blockIdx.x >> 4) % (unsigned)ni))) & 15u);
  const size_t ct = (size_t)((blockIdx.x >> 4) / (unsigned)ni);
  const size_t N = (size_t)c.n, base = (size_t)blk << 10;
  const Mod m = mod_at(c, I);
  const FpTable t = fp_table(c, I);
  const double q = m.qd, qinv = m.qinv;
  double *ltw = dyn + (nl + 1) * lds_words(10);
  const size_t pw = (size_t)nl * N;
  // scalar loads (constant address space): a vector load of these after the transform would expose one more memory latency
  const ABC_CONST_AS DevConst *cst = (const ABC_CONST_AS DevConst *)c.cst;
  const double inv = cst->inv_special_c[I], inv_q = cst->inv_special_cq[I];

  // (1) twiddle table, (2) this wavefront's half-done limb, (3) the operands of this thread's first coefficient pair
  double twv[PER];
  block_twiddles_fetch<10, double, PER>(t.tw, 4, blk, (int)threadIdx.x, NT, twv);
  const bool has_limb = W <= nl;  // wavefront-uniform
  const int Wc = has_limb ? W : 0;
  const double *__restrict__ src = (Wc < nl - 1) ? part + ((ct * (nl + 1) + I) * nl + (Wc < I ? Wc : Wc + 1)) * (size_t)c.ps + base
                                                 : tpart + ((ct * 2 + (Wc - (nl - 1))) * nl + I) * (size_t)c.ps + base;
  const int pk = pack ? pack_kind(m.bits) : 0;  // workgroup-uniform
  u64x2 raw[8];
  if (has_limb) {  // eight loads of one coefficient pair: slot g*8 + k = element k*128 + 2*lane + g (ntt_fwd_tail1024_pairs)
    if (pk == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) raw[k] = *reinterpret_cast<const u64x2 *>(src + (k << 7) + 2 * lane);
    } else if (pk == 1) {
#pragma unroll
      for (int k = 0; k < 8; k++) raw[k] = pack_load_pair<1>(src - base, N, base + (k << 7) + 2 * lane);
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) raw[k] = pack_load_pair<2>(src - base, N, base + (k << 7) + 2 * lane);
    }
  }
  // key words: 16 raw bytes per (digit, component) either way -- the key's fp64 twin where it exists (keyf, workgroup-uniform:
  // the words ARE the doubles), the u64 key otherwise (converted when used, after the transform)
  // digits j0 .. j1 - 1; HALVES: of component comp
  auto load_key = [&](int e, Ops &o, int j0, int j1, int comp) {
    const u64 *kw = keyf ? reinterpret_cast<const u64 *>(keyf) : key;
#pragma unroll
    for (int Jx = 0; Jx < NL; Jx++) {
      if (Jx < j0 || Jx >= j1) continue;
      if constexpr (HALVES) {
        o.k[Jx] = *reinterpret_cast<const u64x2 *>(kw + (((size_t)Jx * 2 + comp) * c.K + I) * N + base + e);
      } else {
        o.k[2 * Jx + 0] = *reinterpret_cast<const u64x2 *>(kw + (((size_t)Jx * 2 + 0) * c.K + I) * N + base + e);
        o.k[2 * Jx + 1] = *reinterpret_cast<const u64x2 *>(kw + (((size_t)Jx * 2 + 1) * c.K + I) * N + base + e);
      }
    }
  };
  auto load_operands = [&](int e, Ops &o) {
    if (MODE == 0) {
      const u64 *pa = opa + ct * 2 * pw + (size_t)I * N + base + e, *pb = opb + ct * 2 * pw + (size_t)I * N + base + e;
      o.a0 = *reinterpret_cast<const u64x2 *>(pa); o.a1 = *reinterpret_cast<const u64x2 *>(pa + pw);
      o.b0 = *reinterpret_cast<const u64x2 *>(pb); o.b1 = *reinterpret_cast<const u64x2 *>(pb + pw);
    } else {
      const u64 *xl = opa + ct * opa_stride + (size_t)I * N;  // whole limb: a rotation gathers across blocks
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const u32 si = galois_ntt_src<GAL>((u32)(base + e + k), gelt, c.logn);
        o.xs[k] = xl[si];
        o.d0s[k] = o.d1s[k] = 0;
        if (opb) {
          const u64 *ad = opb + ct * opb_stride + (size_t)I * N;
          o.d0s[k] = ad[si];
          if (add_c1) o.d1s[k] = ad[pw + si];
        }
      }
      if constexpr (ACC) {  // the thread's own pair of either component: one 16-byte load each
        const u64 *ac = acc + ct * 2 * pw + (size_t)I * N + base + e;
        const u64x2 c0 = *reinterpret_cast<const u64x2 *>(ac), c1 = *reinterpret_cast<const u64x2 *>(ac + pw);
        // canonical residues: each sum is below 2q <= 2^51 (d1s with add_c1 too), exact in fp_from_u64; fp_mul_lazy's |.| <= q
        // plus it is below 3q < 2^52 in fp_to_canon, which centres any such value exactly
        o.d0s[0] += c0.x; o.d0s[1] += c0.y;
        o.d1s[0] += c1.x; o.d1s[1] += c1.y;
      }
    }
  };
  // MAC: the thread's own pair of the plaintext and of acc's component comp, ahead of that component's store.  HALVES takes acc one
  // component per half (four registers instead of eight): the second half's pair is at an index that no store of the first half
  // touches, so `out` may still be `acc`.  (MAC_INNER reads the plaintext pair again in the second half: an L2 hit, four registers
  // less across the first half's store)
  [[maybe_unused]] u64x2 mp = {0, 0}, ma[2] = {{0, 0}, {0, 0}};
  auto load_mac = [&](int e, int comp) {
    if (comp == 0 || MAC_INNER) mp = *reinterpret_cast<const u64x2 *>(mac.plain + ct * mac.plain_stride + (size_t)I * N + base + e);
    if (acc) ma[comp] = *reinterpret_cast<const u64x2 *>(acc + (ct * 2 + comp) * pw + (size_t)I * N + base + e);  // workgroup-uniform
  };
  Ops ops;
  const int e0 = 2 * (int)threadIdx.x;
  if (!HALVES) {
    load_key(e0, ops, 0, NL - LATE, 0);
    load_operands(e0, ops);
    if constexpr (MAC && !MAC_LATE) {
      load_mac(e0, 0);
      load_mac(e0, 1);
    }
  }

  block_twiddles_store<10, double, PER>(ltw, (int)threadIdx.x, NT, twv);
  __syncthreads();
  if (has_limb) {
    double *buf = dyn + W * lds_words(10);
    double xin[16];
    if (pk == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        xin[k] = __longlong_as_double((long long)raw[k].x);
        xin[8 + k] = __longlong_as_double((long long)raw[k].y);
      }
    } else if (pk == 1) {
#pragma unroll
      for (int k = 0; k < 8; k++) pack_decode_pair<1>(raw[k], xin[k], xin[8 + k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) pack_decode_pair<2>(raw[k], xin[k], xin[8 + k]);
    }
    // raw half-done limbs arrive below 4.7 q (four lazy stages from a canonical value): primes of 49 / 50 bits re-centre before
    // the remaining ten stages, smaller ones have the headroom for all fourteen (abc_ntt.hpp, FpK::red); packed ones arrive
    // centred -- wavefront-uniform branch
    if (m.bits >= 49) {
#pragma unroll
      for (int r = 0; r < 16; r++) xin[r] = fp_centre(xin[r], q, qinv);
    }
    ntt_fwd_tail1024_pairs<FpTail>(buf, xin, [&](int, int i, double v) { buf[lds_pad(i)] = v; }, t, m, 4, blk, lane, ltw);
  }
  // HALVES: a wavefront without a limb arrives here straight from the first barrier, so its requests are in flight across the
  // others' transform at no cost in registers; the transforming wavefronts wait for theirs behind the second barrier
  if (HALVES) {
    load_key(e0, ops, 0, NL, 0);
    load_operands(e0, ops);
    if constexpr (MAC && !MAC_INNER) load_mac(e0, 0);
  }
  if (LATE) load_key(e0, ops, NL - LATE, NL, 0);
  if constexpr (MAC && MAC_LATE) {
    load_mac(e0, 0);
    load_mac(e0, 1);
  }
  __syncthreads();
  auto compute_pair = [&](int e, Ops &o, auto twin) {
    constexpr bool TW = decltype(twin)::value;
    auto kd = [](u64 w) { return TW ? __longlong_as_double((long long)w) : fp_from_u64(w); };
    double xd[2], d0[2] = {0.0, 0.0}, d1[2] = {0.0, 0.0};
    auto diagonal = [&]() {  // the digit modulo q_I itself and the terms folded in as q_sp c: everything that depends on a and b
      if (MODE == 0) {
        const double x0[2] = {fp_from_u64(o.a0.x), fp_from_u64(o.a0.y)}, x1[2] = {fp_from_u64(o.a1.x), fp_from_u64(o.a1.y)};
        const double y0[2] = {fp_from_u64(o.b0.x), fp_from_u64(o.b0.y)}, y1[2] = {fp_from_u64(o.b1.x), fp_from_u64(o.b1.y)};
#pragma unroll
        for (int k = 0; k < 2; k++) {
          xd[k] = fp_mulmod(x1[k], y1[k], q, qinv);
          d0[k] = fp_mulmod(x0[k], y0[k], q, qinv);
          d1[k] = fp_mulmod(x0[k], y1[k], q, qinv) + fp_mulmod(x1[k], y0[k], q, qinv);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 2; k++) {
          xd[k] = fp_from_u64(o.xs[k]);
          d0[k] = fp_from_u64(o.d0s[k]);
          d1[k] = fp_from_u64(o.d1s[k]);
        }
      }
    };
    auto digit = [&](int Jx, double *x) {  // Jx != I: finished by wavefront Jx (Jx - 1 past the diagonal)
      const int w = Jx < I ? Jx : Jx - 1;
      const f64x2 v = *reinterpret_cast<const f64x2 *>(dyn + w * lds_words(10) + lds_pad(e));
      x[0] = v.x;
      x[1] = v.y;
    };
    auto finish = [&](int comp, const double *s, const double *d) {  // (sum + q_sp c - NTT(t)) q_sp^-1
      const f64x2 u = *reinterpret_cast<const f64x2 *>(dyn + (nl - 1 + comp) * lds_words(10) + lds_pad(e));
      u64x2 r;
      if constexpr (MAC) {  // acc + plain (.) r
        r.x = fp_mac_canon(fp_mul_lazy(s[0] - u.x, inv, inv_q, q) + d[0], fp_from_u64(mp.x), ma[comp].x, q, qinv);
        r.y = fp_mac_canon(fp_mul_lazy(s[1] - u.y, inv, inv_q, q) + d[1], fp_from_u64(mp.y), ma[comp].y, q, qinv);
      } else {
        r.x = fp_to_canon(fp_mul_lazy(s[0] - u.x, inv, inv_q, q) + d[0], q, qinv);
        r.y = fp_to_canon(fp_mul_lazy(s[1] - u.y, inv, inv_q, q) + d[1], q, qinv);
      }
      *reinterpret_cast<u64x2 *>(out + ((ct * 2 + comp) * nl + I) * N + base + e) = r;
    };
    if constexpr (HALVES) {
      diagonal();  // before the first store: `out` may alias a or b
      // pinned here: left alone the compiler sinks d1's products into the second half and keeps all of a and b alive for them
      // (16 VGPRs instead of 4, and scratch at four limbs)
#pragma unroll
      for (int k = 0; k < 2; k++) asm volatile("" : "+v"(xd[k]), "+v"(d0[k]), "+v"(d1[k]));
      auto half = [&](auto comp, const double *d) {
        double s[2] = {0.0, 0.0};
#pragma unroll
        for (int Jx = 0; Jx < NL; Jx++) {  // at most four products: below the re-centring at Jx == 7
          double x[2] = {xd[0], xd[1]};
          if (Jx != I) digit(Jx, x);
          s[0] += fp_mulmod(x[0], kd(o.k[Jx].x), q, qinv);
          s[1] += fp_mulmod(x[1], kd(o.k[Jx].y), q, qinv);
        }
        if constexpr (MAC_INNER) {
          __builtin_amdgcn_sched_barrier(0);
          load_mac(e, decltype(comp)::value);
        }
        finish(decltype(comp)::value, s, d);
      };
      half(std::integral_constant<int, 0>{}, d0);
      __builtin_amdgcn_sched_barrier(0);  // the second half's requests stay behind the first half's store (78 -> 70 VGPRs at four limbs)
      load_key(e, o, 0, NL, 1);
      if constexpr (MAC && !MAC_INNER) load_mac(e, 1);
      half(std::integral_constant<int, 1>{}, d1);
    } else {
      double s0[2] = {0.0, 0.0}, s1[2] = {0.0, 0.0};
#pragma unroll
      for (int Jx = 0; Jx < NL; Jx++) {
        double x[2];
        if (Jx == I) {
          diagonal();
          x[0] = xd[0];
          x[1] = xd[1];
        } else {
          digit(Jx, x);
        }
        s0[0] += fp_mulmod(x[0], kd(o.k[2 * Jx + 0].x), q, qinv);
        s0[1] += fp_mulmod(x[1], kd(o.k[2 * Jx + 0].y), q, qinv);
        s1[0] += fp_mulmod(x[0], kd(o.k[2 * Jx + 1].x), q, qinv);
        s1[1] += fp_mulmod(x[1], kd(o.k[2 * Jx + 1].y), q, qinv);
        if (Jx == 7) {
#pragma unroll
          for (int k = 0; k < 2; k++) {
            s0[k] = fp_centre(s0[k], q, qinv);
            s1[k] = fp_centre(s1[k], q, qinv);
          }
        }
      }
      finish(0, s0, d0);
      finish(1, s1, d1);
    }
  };
  if (keyf) compute_pair(e0, ops, std::true_type{});  // workgroup-uniform
  else compute_pair(e0, ops, std::false_type{});
}

// over the slots of a.imap
bool split4_main(abc_hip_ctx *c, const MainArgs &a) {
  const KsOperands &o = a.ops;
  if (o.nl < 1 || o.nl > 7) return false;  // nl + 1 transform buffers of 8.5 KiB + the 8 KiB table: LDS allows two workgroups per CU up to nl = 7
  if (a.ni == 0) return true;
  const dim3 grid((unsigned)(o.count * a.ni * 16)), block(512);
  const double *keyf = key_twin_lookup(c, o.key);
  // a.part / a.tpart: raw or packed doubles here (a mixed chain's fp64 limbs: written as doubles by the integer sequence's first steps)
  dispatch_mode(o.mode, o.gather, [&](auto M, auto G) {
    dispatch_nl<1, 7>(o.nl, [&](auto NL) {
      constexpr int MODE = decltype(M)::value, NLV = decltype(NL)::value;
      constexpr bool GAL = decltype(G)::value;
      auto launch = [&](auto H) {
        // with a plaintext up to five limbs: Seq::split14 comes here up to there (route_chunk), and nothing else has one
        dispatch_tail<MODE == 1 && GAL, MODE == 1 && GAL && NLV <= 5>(o, [&](auto... tail) {
          hipLaunchKernelGGL((k_split4_main_fp<MODE, GAL, NLV, decltype(H)::value, typename decltype(tail)::tag...>), grid, block,
                             main_lds_bytes(o.nl, sizeof(double)), a.st, c->dc, (const double *)a.part, (const double *)a.tpart, o.target,
                             o.addend, o.target_stride, o.addend_stride, o.add_c1, o.key, o.out, o.gather, (u32)a.imap, a.ni, a.pack, keyf,
                             tail...);
        });
      };
      // up to four limbs LDS holds three workgroups per CU: the pair phase in two halves fits their registers
      if constexpr (NLV <= 4) {
        if (!c->sw.main_two_per_cu) return launch(std::true_type{});
      }
      launch(std::false_type{});
    });
  });
  return true;
}

// K2a..K2c on the chunk o (the half-done decomposition limbs are in s.dec)
static void launch_split3(abc_hip_ctx *c, hipStream_t st, const FusedScratch &s, const KsOperands &o, const ChunkRoute &k) {
  MainArgs a;
  a.st = st, a.ops = o, a.part = s.dec, a.tpart = s.ksacc, a.ni = o.nl, a.pack = k.pack;
  launch_split_special(st, c, o.count, o.nl, (const double *)s.dec, o.key, (double *)s.tsp);
  hipLaunchKernelGGL(k_split3_pass_fp<14>, dim3((unsigned)(o.count * 2 * 4)), dim3(256), 0, st, c->dc, (const double *)s.tsp,
                     (double *)s.ksacc, o.nl, a.pack);
  if (k.main4 && split4_main(c, a)) return;
  dispatch_mode(o.mode, o.gather, [&](auto M, auto G) { launch_split3_main<decltype(M)::value, decltype(G)::value>(c, a); });
}

// K2a..K3 on the chunk o: operand given by (coef, coef_stride) [+ (ntt, ntt_stride) for CKKS]; key, addend and out are o's
template <int LB>
static int keyswitch_stage(abc_hip_ctx *c, hipStream_t st, const FusedScratch &s, const u64 *coef, size_t coef_stride, const u64 *ntt,
                           size_t ntt_stride, const KsOperands &o, bool fp /* Seq::lds_fp, else lds_int with k's guard / lazy */,
                           const ChunkRoute &k, int dec_ready = 0 /* 1: dec already holds the transformed decomposition limbs */) {
  const size_t N = (size_t)1 << LB, cc = o.count;
  const int nl = o.nl;
  const dim3 block((1 << LB) / 16);
  const bool ckks = (c->scheme == 2);
  const unsigned g2a = (unsigned)(cc * (nl + 1) * nl);
  const unsigned g3 = (unsigned)(cc * 2 * nl);
  // A: the policy of the forward transforms (a type tag); K2c and K3 are still one kernel per arithmetic
  auto run = [&](auto arith, auto lazy) {
    using A = decltype(arith);
    constexpr bool FP = std::is_same_v<A, FpArith>;
    if (!dec_ready)
      hipLaunchKernelGGL((k_fused_ks_decomp_ntt<LB, A, decltype(lazy)::value>), dim3(g2a), block, 0, st, c->dc, coef, coef_stride, s.dec,
                         nl, ckks ? 1 : 0);
    hipLaunchKernelGGL(k_fused_ks_mac, dim3(grid_for(cc * (nl + 1) * (N / 2), 256)), dim3(256), 0, st, c->dc, s.dec,
                       ckks ? ntt : (const u64 *)nullptr, ntt_stride, o.key, s.ksacc, s.tsp, nl, cc);
    hipLaunchKernelGGL((FP ? k_fused_ks_special_intt_fp<LB> : k_fused_ks_special_intt<LB>), dim3((unsigned)(cc * 2)), block, 0, st, c->dc,
                       s.tsp, s.tlast);
    if (!ckks)
      hipLaunchKernelGGL((FP ? k_fused_ks_moddown_bfv_fp<LB> : k_fused_ks_moddown_bfv<LB>), dim3(g3), block, 0, st, c->dc, s.ksacc, s.tlast,
                         o.addend, o.addend_stride, o.add_c1, o.out, nl);
    else if constexpr (FP)
      hipLaunchKernelGGL(k_fused_ks_moddown_fp<LB>, dim3(g3), block, 0, st, c->dc, s.ksacc, s.tlast, o.addend, o.addend_stride, o.add_c1,
                         o.out, nl, (int)(cc * 2));
    else
      hipLaunchKernelGGL((k_fused_ks_moddown<LB, std::is_same_v<A, IntArith<true>>>), dim3(g3), block, 0, st, c->dc, s.ksacc, s.tlast, o.addend,
                         o.addend_stride, o.add_c1, o.out, nl);
  };
  if (fp) run(FpArith{}, std::true_type{});
  else if (k.guard) run(IntArith<true>{}, std::false_type{});
  else if (k.lazy) run(IntArith<false>{}, std::true_type{});
  else run(IntArith<false>{}, std::false_type{});
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

int fork_lanes(abc_hip_ctx *c, int lanes) {
  if (lanes < 2) return 0;
  ABC_HIP_CHECK(hipEventRecord(c->lane_fork, c->stream));
  for (int l = 0; l < lanes; l++) ABC_HIP_CHECK(hipStreamWaitEvent(c->lane[l], c->lane_fork, 0));
  return 0;
}
int join_lanes(abc_hip_ctx *c, int lanes) {
  if (lanes < 2) return 0;
  for (int l = 0; l < lanes; l++) {
    ABC_HIP_CHECK(hipEventRecord(c->lane_join[l], c->lane[l]));
    ABC_HIP_CHECK(hipStreamWaitEvent(c->stream, c->lane_join[l], 0));
  }
  return 0;
}

static int run_isplit(abc_hip_ctx *c, const KsOperands &o) {
  const ChunkPlan p = plan_chunks(c->facts, o.nl, o.count);
  const ChunkRoute k = route_chunk(c->facts, Seq::isplit, o.nl, p.chunk);  // nothing in it depends on the chunk
  return for_each_chunk(c, o.count, p.chunk, p.lanes, isplit_scratch_words(c, o.nl), k.fp_twin ? o.key : nullptr,
                        [&](hipStream_t st, u64 *scratch, size_t off, size_t cc) { return isplit_chunk(c, st, scratch, o.slice(off, cc, (size_t)c->n), k); });
}

// N = 2^15 (abc_kernels_gsplit.hip)
static int run_gsplit15(abc_hip_ctx *c, const KsOperands &o) {
  const ChunkPlan p = plan_chunks(c->facts, o.nl, o.count);
  return for_each_chunk(c, o.count, p.chunk, p.lanes, gsplit_scratch_words(c, o.nl), nullptr,
                        [&](hipStream_t st, u64 *scratch, size_t off, size_t cc) { return gsplit_chunk15(c, st, scratch, o.slice(off, cc, (size_t)c->n)); });
}

// ---- CKKS multiply + relinearise (all is the mode-0 record of the call): Seq::split14 (its scratch limbs are c->dc.ps words
// apart), lds_fp, lds_int ----
template <int LB>
static int run_mul_relin(abc_hip_ctx *c, Seq seq, const KsOperands &all) {
  const size_t N = (size_t)1 << LB;
  const int nl = all.nl;
  const ChunkPlan p = plan_chunks(c->facts, nl, all.count);
  const bool split = seq == Seq::split14, fp = seq != Seq::lds_int;
  const size_t SN = split ? (size_t)c->dc.ps : N;
  const size_t per_ct = fused_scratch_limbs(nl) * SN;
  return for_each_chunk(c, all.count, p.chunk, p.lanes, per_ct, split ? all.key : nullptr, [&](hipStream_t st, u64 *scratch, size_t off, size_t cc) {
    const FusedScratch s = carve(scratch, p.chunk, nl, SN);
    const ChunkRoute k = route_chunk(c->facts, seq, nl, cc);
    const KsOperands o = all.slice(off, cc, N);
    const u64 *a = o.target, *b = o.addend;
    if constexpr (LB == 14) {
      if (split) {
        // lean: the block-wise inverse tails + register cross pass of abc_kernels_gsplit.hip spread over the chip
        if (k.lean)
          gsplit_front14(st, c, o, (double *)s.coef, (double *)s.dec, k.pack);
        else
          hipLaunchKernelGGL(k_split2_tensor_pass0_fp<LB>, dim3((unsigned)(cc * nl)), dim3((1 << LB) / 16), 0, st, c->dc, a, b, (double *)s.dec,
                             nl, (int)k.pack);
        launch_split3(c, st, s, o, k);
        ABC_HIP_CHECK(hipGetLastError());
        return 0;
      }
    }
    if (fp)  // tensor product, inverse transform and the forward transforms of the decomposition in one LDS-resident kernel
      hipLaunchKernelGGL(k_fused_tensor_decomp_fp<LB>, dim3((unsigned)(cc * nl)), dim3((1 << LB) / 16), 0, st, c->dc, a, b, s.c01, s.ntt,
                         s.dec, nl);
    else
      hipLaunchKernelGGL(k_fused_tensor_intt<LB>, dim3((unsigned)(cc * nl)), dim3((1 << LB) / 16), 0, st, c->dc, a, b, s.c01, s.coef, s.ntt, nl);
    // the key switch of the product's third polynomial, (c0, c1) of the product as its addend
    KsOperands ks = o;
    ks.mode = 1, ks.addend = s.c01, ks.addend_stride = 2 * (size_t)nl * N, ks.add_c1 = true;
    return keyswitch_stage<LB>(c, st, s, s.coef, (size_t)nl * N, s.ntt, (size_t)nl * N, ks, fp, k, fp ? 1 : 0);
  });
}

int launch_mul_relin(abc_hip_ctx *c, Seq seq, const u64 *a, const u64 *b, u64 *out, int nl, size_t count) {
  if (!count) return 0;
  KsOperands o;
  o.mode = 0, o.target = a, o.addend = b, o.target_stride = o.addend_stride = 2 * (size_t)nl * c->n;
  o.key = c->d_relin, o.out = out, o.nl = nl, o.count = count;
  switch (seq) {
    case Seq::gsplit15: return run_gsplit15(c, o);
    case Seq::isplit: return run_isplit(c, o);
    case Seq::split14:
    case Seq::lds_fp:
    case Seq::lds_int: return dispatch_logn<10, 14>(c->logn, [&](auto LB) { return run_mul_relin<decltype(LB)::value>(c, seq, o); });
    default: set_error("launch_mul_relin: not a multiply + relinearise sequence of this file"); return 1;
  }
}

// ---- general key switch: Seq::split14, bsplit14, lds_fp, lds_int ----
template <int LB>
static int run_keyswitch(abc_hip_ctx *c, Seq seq, const KsOperands &all) {
  const size_t N = (size_t)1 << LB;
  const int nl = all.nl;
  const bool ckks = (c->scheme == 2);
  const ChunkPlan p = plan_chunks(c->facts, nl, all.count);
  // split sequences (N = 2^14, every key prime below 2^50): CKKS as in run_mul_relin; BFV (coefficient-form operand) the
  // register pass + abc_kernels_gsplit.hip's k_gsplit_special<14, NL, true> (k_bsplit_special8x2 for eight digits) / k_bsplit_tcoef /
  // k_bsplit_finish_big
  const bool splitc = seq == Seq::split14, splitb = seq == Seq::bsplit14, fp = seq != Seq::lds_int;
  const size_t SN = (splitc || splitb) ? (size_t)c->dc.ps : N;
  const size_t per_ct = fused_scratch_limbs(nl) * SN;
  // the split kernels read the key's fp64 twin (BFV: the inner-product kernel)
  return for_each_chunk(c, all.count, p.chunk, p.lanes, per_ct, (splitc || splitb) ? all.key : nullptr, [&](hipStream_t st, u64 *scratch, size_t off, size_t cc) {
    const FusedScratch s = carve(scratch, p.chunk, nl, SN);
    const ChunkRoute k = route_chunk(c->facts, seq, nl, cc);
    const KsOperands o = all.slice(off, cc, N);
    if constexpr (LB == 14) {
      if (splitc) {
        if (k.lean)
          gsplit_front14(st, c, o, (double *)s.coef, (double *)s.dec, k.pack);
        else
          hipLaunchKernelGGL((o.gather ? k_fused_operand_pass0_fp<LB, true, true> : k_fused_operand_pass0_fp<LB, true, false>),
                             dim3((unsigned)(cc * nl)), dim3((1 << LB) / 16), 0, st, c->dc, o.target, o.target_stride, (double *)s.dec, nl, 0,
                             o.gather, 1 | (k.pack ? 2 : 0));
        launch_split3(c, st, s, o, k);
        ABC_HIP_CHECK(hipGetLastError());
        return 0;
      }
      if (splitb) {
        // few ciphertexts in flight (k.per_target): one workgroup per (ct, J, target I) instead of per (ct, J)
        hipLaunchKernelGGL((k_fused_operand_pass0_fp<LB, false, false>), dim3((unsigned)(cc * nl * (k.per_target ? nl + 1 : 1))),
                           dim3((1 << LB) / 16), 0, st, c->dc, o.target, o.target_stride, (double *)s.dec, nl, k.per_target ? 1 : 0, o.gather, 1);
        // inner product + inverse tails for every key prime, then the register-only finish (a rotation's addend g(c0): gathered there)
        return bsplit_back<14>(c, st, (const double *)s.dec, (double *)s.ksacc, o);
      }
    }
    // LDS-resident kernels (smaller rings, wider primes, ABC_HIP_NO_SPLIT)
    const u64 *coef = o.target;
    size_t coef_stride = o.target_stride;
    if (ckks) {  // operand arrives in NTT form: coefficient form via one in-LDS inverse transform per limb
      hipLaunchKernelGGL((fp ? k_fused_operand_intt<LB, FpArith> : k_fused_operand_intt<LB, IntArith<true>>), dim3((unsigned)(cc * nl)),
                         dim3((1 << LB) / 16), 0, st, c->dc, o.target, o.target_stride, s.coef, nl);
      coef = s.coef;
      coef_stride = (size_t)nl * N;
    }
    return keyswitch_stage<LB>(c, st, s, coef, coef_stride, o.target, o.target_stride, o, fp, k, 0);
  });
}

// what the kernels gather with: CKKS (NTT form) the element itself, BFV (coefficient form) its inverse mod 2N
static u32 gather_elt(const KsOperands &o, int scheme, size_t N) {
  return (scheme == 2 || !o.gelt) ? o.gelt : (u32)host::invmod(o.gelt, 2 * (uint64_t)N);
}

int launch_keyswitch(abc_hip_ctx *c, const KsRoute &r, const KsOperands &in) {
  if (!in.count) return 0;
  if (in.gelt && !seq_folds_permutation(c->facts, r)) { set_error("launch_keyswitch: this sequence folds no permutation"); return 1; }
  if (in.plain ? !(in.gelt && seq_takes_plain(c->facts, r, in.nl))
               : in.acc && !(in.gelt && seq_takes_acc(c->facts, r, in.nl))) {
    set_error("launch_keyswitch: a second addend or a plaintext needs a folded permutation and a sequence that takes one");
    return 1;
  }
  KsOperands o = in;
  o.mode = 1, o.gather = gather_elt(o, c->scheme, (size_t)c->n);
  switch (r.seq) {
    case Seq::gsplit15: return run_gsplit15(c, o);
    case Seq::isplit: return run_isplit(c, o);
    case Seq::bsplit_big: return bsplit_big(c, o);  // BFV, coefficient form: the signed permutation folded into the first step's load and the last step's addend
    case Seq::generic: return keyswitch_generic(c, r.front, o);
    case Seq::split14:
    case Seq::bsplit14:
    case Seq::lds_fp:
    case Seq::lds_int: return dispatch_logn<10, 14>(c->logn, [&](auto LB) { return run_keyswitch<decltype(LB)::value>(c, r.seq, o); });
    default: set_error("launch_keyswitch: not a key-switch sequence"); return 1;
  }
}

}  // namespace abc
