// abc_route.hpp -- which kernel sequence a call takes.  Plain C++17: no HIP header, no pointer to device memory, so the whole
// table runs in a host test (tests/cpp/test_route.cpp) and behind abc_hip_route.
//
// One pure function per operation maps (context facts, switches, nl, aliasing) to a named route; one more maps (route, nl,
// ciphertexts in the chunk) to the per-chunk choices.  The dispatchers (abc_context.hip, abc_kernels_fused.hip,
// abc_kernels_eval.hip, abc_kernels_bfv.hip) switch over the result and decide nothing themselves.  DESIGN.md section 3b holds
// the same table in prose, with the strings format() writes.
//
// Not part of a route: whether a key's fp64 twin or Shoup mirror exists.  That is a property of a buffer (ABC_HIP_NO_KEY_TWIN and
// allocation success, key_twin_lookup in abc_buffers.hip), looked up at the launch; the kernels take either form.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace abc {

// Path switches (A/B timing and the parity tests of every fallback): the ABC_HIP_* environment variables are read ONCE, when
// the context is created (abc_hip_ctx_reload_env re-reads them), never on the per-operation path.
struct Switches {
  bool no_fused = false, no_split = false, no_split4 = false, no_isplit = false, no_gsplit = false, no_lean_front = false, no_bsplit = false, no_mixed = false, no_pack = false, no_key_twin = false, no_bmul = false, no_iks = false, no_tensor_intt = false;
  bool no_galois_fusion = false;
  bool no_rotate_add_fusion = false;  // ABC_HIP_NO_ROTATE_ADD_FUSION: rotate_add as a rotation into an arena, then the add kernel
  bool no_rotate_mac_fusion = false;  // ABC_HIP_NO_ROTATE_MAC_FUSION: rotate_mac_plain as a rotation into an arena, multiply_plain on it, then the add kernel
  bool no_mulplain_rescale_fusion = false;  // ABC_HIP_NO_MULPLAIN_RESCALE_FUSION: multiply_plain_rescale as multiply_plain into an arena, then rescale
  bool no_tensor_sum = false;  // ABC_HIP_NO_TENSOR_SUM: multiply_sum / mul_sum_relin form every product on its own (tensor into an arena, then the add kernel)
  bool no_plain_sum_rescale_fusion = false;  // ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION: multiply_plain_sum_rescale (and the inner sums of diag_matvec_bsgs_rescale) as multiply_plain_sum into an arena, then rescale
  bool no_plain_mac_sum = false;  // ABC_HIP_NO_PLAIN_MAC_SUM: multiply_plain_sum (and the inner sums of diag_matvec_bsgs) as multiply_plain into an arena, then the add kernel, per term
  bool no_const_mac_sum = false;  // ABC_HIP_NO_CONST_MAC_SUM: multiply_const_sum (and the last step of ckks_poly_eval) as a filled constant plaintext, mod_switch copies, multiply_plain and the add kernel, per term
  int const_sum_rescale_fused = -1;  // ABC_HIP_CONST_SUM_RESCALE_FUSED=1 / =0: multiply_const_sum_rescale on its fused pair wherever the pair can run / nowhere (tests, A/B); unset: the measured rule of route_const_sum_rescale
  bool main_two_per_cu = false;  // ABC_HIP_MAIN_TWO_PER_CU: k_split4_main_fp in its one-piece pair phase at nl <= 4 (same step, same route: a form of the kernel)
  bool host_sampling = false;  // ABC_HIP_HOST_SAMPLING: the keyed entries (the OS-keyed ones call them) draw with the host twin of the keyed spec (no route depends on it)
  size_t chunk = 0, few_limbs = 48, lean_limit = 96, bfv_scratch_mb = 0, pass0_target_limit = 128;
  int lanes = 2;
  int plain_sum_rescale_terms = -1;  // ABC_HIP_PLAIN_SUM_RESCALE_TERMS (0 .. 8): the fused sum-rescale pair at EVERY batch and term count, taking at most that many terms (A/B runs, parity tests); unset: the measured rule of route_plain_sum_rescale
};

// prime widths the kernels are exact for (abc_ntt.hpp: fp_ok, unguarded_ok)
constexpr unsigned kFpBits = 50;         // fp64 transforms
constexpr unsigned kLazyBits = 55;       // 4 products of a (< 64q) operand with a key residue stay below 2^(k+63)
constexpr unsigned kUnguardedBits = 57;  // unguarded butterflies: 64 q <= 2^64
constexpr unsigned kIsplitBits = 60;     // the integer split kernels

// scratch limbs per ciphertext of the LDS-resident and N = 2^14 split sequences (carve, abc_kernels_fused.hip)
constexpr size_t fused_scratch_limbs(int nl) { return (size_t)nl * (nl + 1) + 6 * (size_t)nl + 4; }

// Everything a route depends on besides the call's own arguments.  Filled when the context is created and by
// abc_hip_ctx_reload_env (primes never change afterwards); finish() derives what the routes ask per call.
struct RouteFacts {
  int scheme = 0, logn = 0, K = 0, L = 0, nB = 0;  // scheme 1 BFV, 2 CKKS; K key primes (bits[K-1]: the special prime), L data limbs
  bool use_fp = true, behz_fp = false;
  int big_block_log = 12;
  unsigned char bits[17] = {};  // width of key prime j
  Switches sw;
  // derived
  unsigned widest = 0;   // widest key prime
  uint32_t fp_mask = 0;  // bit j: key prime j is fp64-capable (whatever use_fp says)
  bool all_fp = false;   // fp64 transforms throughout: use_fp and every key prime below 2^50
  bool guard = false;    // some key prime needs the guarded butterflies
  bool lazy = false;     // unguarded, and the inner product may accumulate lazily
  void finish() {
    widest = 0;
    fp_mask = 0;
    for (int j = 0; j < K; j++) {
      if (bits[j] > widest) widest = bits[j];
      if (bits[j] <= kFpBits) fp_mask |= 1u << j;
    }
    all_fp = use_fp && widest <= kFpBits;
    guard = widest > kUnguardedBits;
    lazy = widest <= kLazyBits;
  }
  uint32_t fp_data_mask(int nl) const { return fp_mask & ((1u << nl) - 1u); }  // the first nl data primes
  bool data_fp(int nl) const { return fp_data_mask(nl) == (1u << nl) - 1u; }
  bool special_fp() const { return K > 0 && ((fp_mask >> (K - 1)) & 1u); }
};

// ---- the sequences ----
enum class Seq {
  split14,     // CKKS, N = 2^14, fp64: tensor / operand pass 0 (lean or fat), special, pass, main (split4 or split3)
  gsplit15,    // CKKS, N = 2^15, fp64 (abc_kernels_gsplit.hip)
  isplit,      // CKKS, N = 2^14 / 2^15, a prime above 2^50: integer split kernels, fp64 for the limbs in fpmask (abc_kernels_isplit.hip)
  bsplit14,    // BFV, N = 2^14, fp64: operand pass 0 + bsplit_back<14>
  bsplit_big,  // BFV, N = 2^13 / 2^15 / 2^16, fp64 (bsplit_big)
  lds_fp,      // LDS-resident limbs, fp64
  lds_int,     // LDS-resident limbs, integers (guard / lazy)
  bmul,        // BFV multiply + relinearise in one split sequence (abc_kernels_bmul.hip)
  generic      // the one-kernel-per-step sequences (abc_kernels_eval.hip, abc_kernels_bfv.hip)
};
enum class KsFront { plain, fp, iks };     // generic key switch: k_ks_expand + transforms / fp64 strided expand / k_iks_pass0 + k_iks_special
enum class BfvMul { behz, split, big };    // BFV multiply alone: generic BEHZ kernels / bmul_split on lanes (2^14) / bmul_big
enum class Rescale { generic, fp, mixed };

struct KsRoute {
  Seq seq;
  KsFront front;  // seq == generic only
};
struct MulRoute {
  Seq seq;
  BfvMul mul;  // seq == generic on BFV: how the size-3 product is formed (CKKS: launch_ckks_tensor)
  KsRoute ks;  // seq == generic: the key switch that follows
};
struct RotRoute {
  bool fold;  // the permutation is folded into the key switch `ks`; otherwise k_galois first, then `ks`
  KsRoute ks;
};
struct RotTailRoute {
  RotRoute rot;
  // what follows the rotation (a second ciphertext to add; a plaintext to multiply by, then the second ciphertext) is an operand of
  // the key switch's last kernel; otherwise rotate into an arena, then multiply_plain there where there is a plaintext, then add
  bool fused;
};
using RotAddRoute = RotTailRoute;  // per operation, as tests/cpp name it
using RotMacRoute = RotTailRoute;
struct RescaleRoute {
  Rescale kind;
  uint32_t fpmask;  // mixed: limbs that take the fp64 butterflies
};
struct MulPlainRescaleRoute {
  RescaleRoute rescale;  // the rescale, out of place
  bool fused;            // the plaintext product is formed in that rescale's loads; otherwise multiply_plain into an arena, then the rescale on it
};
// relinearize(sum of K ciphertext products): the size-3 sum lands in an arena, then the key switch of the level
struct MulSumRoute {
  KsRoute ks;
  bool sum;  // CKKS: one K-term tensor-sum kernel (k_ckks_tensor_sum); otherwise each product by the multiply of the scheme into a second arena, then the add kernel
};

// a matrix-vector product by diagonals, baby-step giant-step: the baby rotations (plain rotations, out of place, into an arena), one
// plaintext multiply-accumulate sum per giant step, then addend + rotate(inner sum) with d_out as addend and output
struct MatvecBsgsRoute {
  RotRoute baby;
  bool macsum;         // one K-term kernel (k_ckks_plain_mac_sum); otherwise multiply_plain into an arena and the add kernel, per term
  RotTailRoute giant;  // route_rotate_add, out of place
};

namespace route_detail {
inline bool gsplit_ok(const RouteFacts &f, int nl) {
  return f.logn == 15 && f.scheme == 2 && f.use_fp && !f.sw.no_gsplit && nl >= 1 && nl <= 15 && f.widest <= kFpBits;
}
inline bool bsplit_ok(const RouteFacts &f, int nl) {
  return f.logn == 14 && f.scheme == 1 && f.use_fp && !f.sw.no_bsplit && nl >= 1 && nl <= 8 && f.widest <= kFpBits;
}
inline bool bsplit_big_ok(const RouteFacts &f, int nl) {
  return (f.logn == 13 || f.logn == 15 || f.logn == 16) && f.scheme == 1 && f.use_fp && !f.sw.no_bsplit && !f.sw.no_gsplit && nl >= 1 &&
         nl <= 8 && f.widest <= kFpBits;
}
inline bool isplit_ok(const RouteFacts &f, int nl) {
  if ((f.logn != 14 && f.logn != 15) || f.scheme != 2 || f.sw.no_fused || f.sw.no_split || f.sw.no_isplit || nl < 1 ||
      nl > (f.logn == 15 ? 15 : 7))
    return false;
  if (f.logn == 15 && f.sw.no_gsplit) return false;  // one switch turns both split sequences of that ring off (A/B, tests)
  return f.widest <= kIsplitBits;
}
inline bool bmul_shape(const RouteFacts &f, int limbs) {
  return f.scheme == 1 && f.use_fp && f.behz_fp && !f.sw.no_bmul && !f.sw.no_split && !f.sw.no_fused && f.L == limbs && f.nB == limbs &&
         f.K == f.L + 1;
}
inline bool bmul_relin_ok(const RouteFacts &f) {
  if (f.logn == 13) return bmul_shape(f, 4) && bsplit_big_ok(f, f.L);  // BFVDefault(8192)
  return f.logn == 14 && bmul_shape(f, 8) && bsplit_ok(f, f.L);
}
// the choice among the sequences with LDS-resident or N = 2^14 split limbs (rings 2^10 .. 2^14)
inline Seq lds_seq(const RouteFacts &f, int nl, bool mul) {
  const bool ckks = f.scheme == 2;
  if (f.logn == 14 && ckks && !f.all_fp && isplit_ok(f, nl)) return Seq::isplit;
  if (f.logn == 14 && ckks && f.all_fp && !f.sw.no_split && nl <= 12) return Seq::split14;
  if (!mul && f.logn == 14 && !ckks && !f.sw.no_split && bsplit_ok(f, nl)) return Seq::bsplit14;
  return f.all_fp ? Seq::lds_fp : Seq::lds_int;
}
}  // namespace route_detail

// the front of the generic key switch at level nl
inline KsFront route_ks_front(const RouteFacts &f, int nl) {
  if (f.logn > 14 && f.use_fp && f.data_fp(nl) && f.special_fp()) return KsFront::fp;
  if ((f.logn == 15 || f.logn == 16) && !f.sw.no_iks && f.big_block_log == 12) return KsFront::iks;
  return KsFront::plain;
}

// relinearise and plain key switch
inline KsRoute route_keyswitch(const RouteFacts &f, int nl) {
  using namespace route_detail;
  const KsRoute generic{Seq::generic, route_ks_front(f, nl)};
  if (f.logn == 15 && gsplit_ok(f, nl)) return {Seq::gsplit15, KsFront::plain};
  if (f.logn == 15 && f.scheme == 2 && !f.all_fp && isplit_ok(f, nl)) return {Seq::isplit, KsFront::plain};
  if (bsplit_big_ok(f, nl)) return {Seq::bsplit_big, KsFront::plain};
  if (f.logn > 14 || f.logn < 10 || f.sw.no_fused) return generic;
  return {lds_seq(f, nl, false), KsFront::plain};
}

inline BfvMul route_bfv_multiply(const RouteFacts &f) {
  using namespace route_detail;
  if (f.logn == 14) return bmul_relin_ok(f) ? BfvMul::split : BfvMul::behz;
  if (f.logn == 13) return bmul_shape(f, 4) ? BfvMul::big : BfvMul::behz;
  return ((f.logn == 15 || f.logn == 16) && bmul_shape(f, 8) && !f.sw.no_gsplit && f.big_block_log == 12) ? BfvMul::big : BfvMul::behz;
}

inline MulRoute route_mul_relin(const RouteFacts &f, int nl) {
  using namespace route_detail;
  const KsRoute none{Seq::generic, KsFront::plain};
  if (f.scheme == 2) {
    if (f.logn == 15 && gsplit_ok(f, nl)) return {Seq::gsplit15, BfvMul::behz, none};
    if (f.logn == 15 && !f.all_fp && isplit_ok(f, nl)) return {Seq::isplit, BfvMul::behz, none};
    if (f.logn <= 14 && f.logn >= 10 && !f.sw.no_fused) return {lds_seq(f, nl, true), BfvMul::behz, none};
    return {Seq::generic, BfvMul::behz, route_keyswitch(f, nl)};
  }
  if (bmul_relin_ok(f)) return {Seq::bmul, BfvMul::split, none};
  return {Seq::generic, route_bfv_multiply(f), route_keyswitch(f, nl)};
}

// ---- what the launch code of a sequence can do (launch_keyswitch checks a call against these, once) ----
// the Galois gather folded into the first and the last kernels: the CKKS split sequences; BFV: the split sequences and the
// fused integer front of the big rings (k_iks_pass0 / k_iks_finish).  The LDS-resident kernels take the permuted ciphertext
inline bool seq_folds_permutation(const RouteFacts &f, const KsRoute &r) {
  const Seq s = r.seq;
  if (f.scheme == 2) return s == Seq::split14 || s == Seq::isplit || s == Seq::gsplit15;
  return s == Seq::bsplit14 || s == Seq::bsplit_big || (s == Seq::generic && r.front == KsFront::iks);
}
// a second, ungathered ciphertext as one more operand of the last kernel (k_split4_main_fp / k_split3_main_fp, k_gsplit_main up to
// seven limbs -- k_gsplit_main_deep does not -- k_bsplit_finish_big / k_bsplit_finish_lds)
inline bool seq_takes_acc(const RouteFacts &, const KsRoute &r, int nl) {
  const Seq s = r.seq;
  return s == Seq::split14 || s == Seq::bsplit14 || s == Seq::bsplit_big || (s == Seq::gsplit15 && nl <= 7);
}
// a plaintext [nl][N] that multiplies the finished pair, and a second ciphertext added to the product, in the last kernel
// (k_split4_main_fp / k_split3_main_fp, k_gsplit_main up to seven limbs): the CKKS sequences among seq_takes_acc's -- a BFV
// plaintext product needs transforms
inline bool seq_takes_plain(const RouteFacts &, const KsRoute &r, int nl) {
  return r.seq == Seq::split14 || (r.seq == Seq::gsplit15 && nl <= 7);
}

// one Galois element at level nl: the key switch of the level, with the permutation folded into it where its sequence gathers
inline RotRoute route_rotate(const RouteFacts &f, int nl, bool in_place) {
  const KsRoute ks = route_keyswitch(f, nl);
  bool fold = !in_place && !f.sw.no_galois_fusion && seq_folds_permutation(f, ks);
  // bsplit_big is chosen whatever these two say, but a rotation under either switch takes the permuted ciphertext (A/B, tests)
  if (ks.seq == Seq::bsplit_big && (f.sw.no_split || f.sw.no_fused)) fold = false;
  return {fold, ks};
}

// addend + one Galois element at level nl; in_place: d_out == d_in (the gather reads whole limbs of d_in, so that call is never
// fused).  `rot` is the rotation either way: the unfused sequence rotates into an arena, never in place, whatever d_out is.
inline RotTailRoute route_rotate_add(const RouteFacts &f, int nl, bool in_place) {
  const RotRoute rot = route_rotate(f, nl, false);
  return {rot, rot.fold && seq_takes_acc(f, rot.ks, nl) && !in_place && !f.sw.no_rotate_add_fusion};
}

// addend + plain (.) one Galois element at level nl (CKKS); in_place and `rot` as in route_rotate_add.  The unfused sequence
// rotates into an arena, multiplies there in place, then adds.
inline RotTailRoute route_rotate_mac(const RouteFacts &f, int nl, bool in_place) {
  const RotRoute rot = route_rotate(f, nl, false);
  return {rot, rot.fold && seq_takes_plain(f, rot.ks, nl) && !in_place && !f.sw.no_rotate_mac_fusion};
}

inline RescaleRoute route_rescale(const RouteFacts &f, int nl, bool in_place) {
  if (f.logn > 14 || f.logn < 10 || in_place || f.sw.no_fused) return {Rescale::generic, 0u};
  if (f.use_fp && f.data_fp(nl)) return {Rescale::fp, 0u};
  if (f.sw.no_isplit) return {Rescale::generic, 0u};
  return {Rescale::mixed, (f.use_fp && !f.sw.no_mixed) ? f.fp_data_mask(nl) : 0u};  // a prime above 2^50 in the chain
}

// rescale(ct (.) plain) at level nl (CKKS): the LDS-resident rescale kernels take the plaintext as an operand of their loads; the
// generic sequence does not
inline MulPlainRescaleRoute route_mulplain_rescale(const RouteFacts &f, int nl) {
  const RescaleRoute r = route_rescale(f, nl, false);
  return {r, r.kind != Rescale::generic && !f.sw.no_mulplain_rescale_fusion};
}

// sum of products at level nl, then one relinearisation.  BFV's product is BEHZ: the sum has to be taken behind its floor to stay
// bit-identical to multiply + add, so it goes term by term
inline MulSumRoute route_mul_sum(const RouteFacts &f, int nl) {
  return {route_keyswitch(f, nl), f.scheme == 2 && !f.sw.no_tensor_sum};
}

// (addend or 0) + sum of K plaintext products at level nl (CKKS): the K-term kernel at every ring, chain and level
inline bool route_plain_mac_sum(const RouteFacts &f, int) { return f.scheme == 2 && !f.sw.no_plain_mac_sum; }
// multiply_const_sum: the K-term scalar-weighted kernel (k_ckks_const_mac_sum), or the composed sequence per term
inline bool route_const_mac_sum(const RouteFacts &f, int) { return f.scheme == 2 && !f.sw.no_const_mac_sum; }

// rescale((addend or 0) + sum of K plaintext products) at level nl (CKKS), `polys` = count * size polynomials.  Fused: the K-term forms
// of the LDS-resident rescale kernels form the sum of the last `fused_terms` terms (and the carried value) in their loads; the terms
// before those go through multiply_plain_sum into an arena, which is the carry.  Separate: the whole sum into the arena, then the
// rescale.  Fused needs an LDS-resident rescale and neither ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION nor ABC_HIP_NO_PLAIN_MAC_SUM (the
// per-term form of the sum).  Among those shapes the measurement decides (profiles/plain_sum_rescale_ab.log):
// the pair beats multiply_plain_sum + rescale for sums of up to kPlainSumRescaleTerms = 4 terms -- every term in the pair, no
// leading launch -- once R1 has a workgroup per CU and 2^20 coefficients to transform; at 6 terms and above, with a leading
// launch at any number of fused terms (8, 4, 2, the carry alone), and on small batches (R1 is one workgroup per polynomial; the
// streaming kernel spreads the same loads over every CU) the two steps are as fast or faster.  ABC_HIP_PLAIN_SUM_RESCALE_TERMS=t
// takes the measurement out: fused at every batch and term count, at most t terms in the pair.
constexpr int kPlainSumRescaleTerms = 4;
constexpr size_t kPlainSumRescaleMinPolys = 256, kPlainSumRescaleMinCoeffs = (size_t)1 << 20;
struct PlainSumRescaleRoute {
  RescaleRoute rescale;  // the rescale, out of place
  bool fused;
  int fused_terms;  // fused: the most terms the pair takes
};
// polys / n_terms default to a large batch and one term: "could this level fuse at all"
inline PlainSumRescaleRoute route_plain_sum_rescale(const RouteFacts &f, int nl, size_t polys = (size_t)1 << 30, int n_terms = 1) {
  const RescaleRoute r = route_rescale(f, nl, false);
  if (r.kind == Rescale::generic || f.sw.no_plain_sum_rescale_fusion || f.sw.no_plain_mac_sum) return {r, false, 0};
  if (f.sw.plain_sum_rescale_terms >= 0) return {r, true, f.sw.plain_sum_rescale_terms < 8 ? f.sw.plain_sum_rescale_terms : 8};
  const bool wins = n_terms <= kPlainSumRescaleTerms && polys >= kPlainSumRescaleMinPolys && (polys << f.logn) >= kPlainSumRescaleMinCoeffs;
  return {r, wins, kPlainSumRescaleTerms};
}
// multiply_const_sum_rescale (and the last step of ckks_poly_eval): the sum formed in the loads of the two LDS-resident rescale kernels
// (k_constsum_rescale_*: fused), or multiply_const_sum into an arena and then the rescale (separate).  The pair CAN run where the
// rescale is LDS-resident (rings up to 2^14; not ABC_HIP_NO_FUSED, nor ABC_HIP_NO_ISPLIT on a chain with a prime above 2^50), on 1 ..
// kConstSumRescaleTerms terms that all sit at level nl (`raised`: some term is held higher -- another stride, which only the
// streaming kernel reads), and not under ABC_HIP_NO_CONST_MAC_SUM.  Within that, ABC_HIP_CONST_SUM_RESCALE_FUSED=1 / =0 force it on
// and off; unset, the measured rule (profiles/const_sum_ab.log).  It started from route_plain_sum_rescale's -- four terms, 256
// polynomials, 2^20 coefficients -- and the measurement moved one bound: with one load per coefficient and term instead of two the
// pair is faster than the two steps at EVERY shape measured up to four terms, down to 64 polynomials (N = 2^14, batch 32),
// where the plaintext pair loses; all of those shapes have 2^20 coefficients or more, so that bound stays, unmeasured below.
constexpr int kConstSumRescaleTerms = 4;
constexpr size_t kConstSumRescaleMinPolys = 64, kConstSumRescaleMinCoeffs = (size_t)1 << 20;
struct ConstSumRescaleRoute {
  RescaleRoute rescale;  // the rescale, out of place
  bool fused;
};
inline ConstSumRescaleRoute route_const_sum_rescale(const RouteFacts &f, int nl, size_t polys, int n_terms, bool raised) {
  const RescaleRoute r = route_rescale(f, nl, false);
  if (r.kind == Rescale::generic || f.sw.no_const_mac_sum || raised || n_terms < 1 || n_terms > kConstSumRescaleTerms) return {r, false};
  if (f.sw.const_sum_rescale_fused >= 0) return {r, f.sw.const_sum_rescale_fused != 0};
  return {r, polys >= kConstSumRescaleMinPolys && (polys << f.logn) >= kConstSumRescaleMinCoeffs};
}
// terms of a K-term sum that the streaming kernel sums into the arena first: whole launches of terms_per_launch, as few as leave the
// fused pair at most fused_terms
inline int plain_sum_rescale_lead(int n_terms, int fused_terms, int terms_per_launch = 8) {
  if (fused_terms < 0) fused_terms = 0;
  if (fused_terms > terms_per_launch) fused_terms = terms_per_launch;
  if (n_terms <= fused_terms) return 0;
  const int lead = (n_terms - fused_terms + terms_per_launch - 1) / terms_per_launch * terms_per_launch;
  return lead < n_terms ? lead : n_terms;
}

// the matvec with the rescale behind every inner sum: baby rotations at nl, one sum-rescale per giant step, giant rotate_adds at nl - 1
struct MatvecBsgsRescaleRoute {
  RotRoute baby;
  PlainSumRescaleRoute sum;
  RotTailRoute giant;  // route_rotate_add at nl - 1, out of place
};
// polys: of one group's inner sum; n_baby: its terms
inline MatvecBsgsRescaleRoute route_matvec_bsgs_rescale(const RouteFacts &f, int nl, size_t polys = (size_t)1 << 30, int n_baby = 1) {
  return {route_rotate(f, nl, false), route_plain_sum_rescale(f, nl, polys, n_baby), route_rotate_add(f, nl - 1, false)};
}

inline MatvecBsgsRoute route_matvec_bsgs(const RouteFacts &f, int nl) {
  return {route_rotate(f, nl, false), route_plain_mac_sum(f, nl), route_rotate_add(f, nl, false)};
}

// (addend or 0) + sum of K plaintext products with ONE inverse transform (BFV, abc_hip_bfv_multiply_plain_sum and the inner sums of
// abc_hip_bfv_diag_matvec_bsgs), from ring, prime widths and batch only:
//   fused       k_bfv_plain_sum_fp: forward transforms, products, sum and the inverse transform of a limb in one workgroup; rings
//               2^10 .. 2^14 with every data prime below 2^50 -- where bfv_multiply_plain takes its fused kernel
//   ntt_domain  transforms by the stand-alone launches, the sum by k_ckks_plain_mac_sum on NTT-form data: N >= 2^15, a prime of
//               2^50 or above, no fp64, ABC_HIP_NO_FUSED, and at N = 2^14 a batch of at most kBfvPlainSumSmall ciphertext limbs
//               (counted at size 2), where the stand-alone transforms spread a limb over many workgroups (bfv_multiply_plain's rule)
enum class BfvPlainSum { fused, ntt_domain };
constexpr size_t kBfvPlainSumSmall = 48;
inline BfvPlainSum route_bfv_plain_sum(const RouteFacts &f, size_t count) {
  const bool fp = f.use_fp && !f.sw.no_fused && f.logn >= 10 && f.logn <= 14 && f.L >= 1 && f.data_fp(f.L);
  if (fp && (f.logn < 14 || count * 2 * (size_t)f.L > kBfvPlainSumSmall)) return BfvPlainSum::fused;
  return BfvPlainSum::ntt_domain;
}
// polynomials per ciphertext the call keeps in context arenas.  fused: the NTT-domain partial sum between two launches, where the
// terms do not fit one (terms_per_launch = 8: kBfvPlainSumTerms, and kPlainMacTerms on the other route).  ntt_domain: the forward
// transforms of up to eight coefficient-form terms, and the sum where an addend keeps it out of d_out
inline size_t bfv_plain_sum_arena_polys(BfvPlainSum r, bool ct_ntt, int n_terms, int size, bool addend, int terms_per_launch = 8) {
  if (r == BfvPlainSum::fused) return n_terms > terms_per_launch ? (size_t)size : 0;
  const int per = n_terms < terms_per_launch ? n_terms : terms_per_launch;
  return (ct_ntt ? 0 : (size_t)per * size) + (addend ? (size_t)size : 0);
}
// ciphertexts per group of that call: as many as keep polys_per_ct polynomials of L limbs each within 4 GiB (plan_chunks' cap)
inline size_t bfv_plain_sum_group(const RouteFacts &f, size_t count, size_t polys_per_ct) {
  if (!polys_per_ct || !count) return count;
  const size_t per_ct_bytes = polys_per_ct * (size_t)f.L * ((size_t)1 << f.logn) * 8;
  const size_t cap = ((size_t)4 << 30) / per_ct_bytes;
  const size_t group = cap ? cap : 1;
  return group < count ? group : count;
}
// the BFV matvec by diagonals, baby-step giant-step: the baby rotations into an arena and ONE forward transform of the slabs, one
// NTT-form inner sum per giant step (no forward transform at all), then addend + rotate(inner sum)
struct BfvMatvecBsgsRoute {
  RotRoute baby;
  BfvPlainSum sum;     // of an inner sum over `group` ciphertexts
  RotTailRoute giant;  // route_rotate_add, out of place
};
inline BfvMatvecBsgsRoute route_bfv_matvec_bsgs(const RouteFacts &f, size_t group) {
  return {route_rotate(f, f.L, false), route_bfv_plain_sum(f, group), route_rotate_add(f, f.L, false)};
}

// ---- per chunk ----
struct ChunkPlan {
  size_t chunk;
  int lanes;
};
// Chunks alternate between two internal streams so that the HBM-streaming kernels of one chunk overlap the ALU-bound
// transforms of the other; measured on MI355X: 256-pair chunks on two lanes beat one 512-pair chunk per lane.
inline ChunkPlan plan_chunks(const RouteFacts &f, int nl, size_t count) {
  ChunkPlan p{f.sw.chunk, f.sw.lanes};
  if (count <= 8) p.lanes = 1;
  if (!p.chunk) {
    const size_t per_ct_bytes = fused_scratch_limbs(nl) * ((size_t)1 << f.logn) * 8;
    const size_t cap = ((size_t)4 << 30) / per_ct_bytes / (size_t)p.lanes;  // scratch capped at 4 GiB
    p.chunk = (count + p.lanes - 1) / p.lanes;
    if (p.chunk > 128) p.chunk = 128;  // measured: 128 > 256 > 64 > 512 (+2 / 0 / -0.5 / -1.5 %)
    if (p.chunk > cap) p.chunk = cap;
    if (p.chunk < 1) p.chunk = 1;
  }
  if (p.chunk > count) p.chunk = count;
  return p;
}
// A call that keeps polys_per_ct polynomials per ciphertext in an arena walks the batch in groups of ciphertexts: a multiple of
// chunk * lanes (the key switch inside a group chunks as a whole call of that many would), as many of them as keep the arena within
// the 4 GiB of plan_chunks' cap; with ABC_HIP_CHUNK set, exactly chunk * lanes.  mul_sum_relin: its size-3 sum
inline size_t arena_group(const RouteFacts &f, int nl, size_t count, size_t polys_per_ct) {
  const ChunkPlan p = plan_chunks(f, nl, count);
  const size_t unit = p.chunk * (size_t)p.lanes;
  if (f.sw.chunk || unit >= count) return unit < count ? unit : count;
  const size_t per_ct_bytes = polys_per_ct * (size_t)nl * ((size_t)1 << f.logn) * 8;
  const size_t units = ((size_t)4 << 30) / per_ct_bytes / unit;
  const size_t group = unit * (units ? units : 1);
  return group < count ? group : count;
}
inline size_t mul_sum_group(const RouteFacts &f, int nl, size_t count) { return arena_group(f, nl, count, 3); }
// diag_matvec_bsgs keeps n_baby rotated ciphertexts per input in an arena: the same rule with 2 * n_baby polynomials per ciphertext
inline size_t matvec_bsgs_group(const RouteFacts &f, int nl, size_t count, int n_baby) {
  return arena_group(f, nl, count, 2 * (size_t)(n_baby > 0 ? n_baby : 1));
}
// the choices that depend on the cc ciphertexts of one chunk (a ragged last chunk may differ from the others); fields a
// sequence does not read stay false / 0
struct ChunkRoute {
  bool lean = false;        // split14: block-wise front (gsplit_front14) instead of the 139 KiB tensor / operand kernel
  bool pack = false;        // split14: packed half-done limbs (abc_ntt.hpp); only k_split4_main_fp reads them
  bool main4 = false;       // split14: k_split4_main_fp, else k_split3_main_fp
  bool per_target = false;  // bsplit14: one workgroup per (ct, J, target I) in pass 0
  bool guard = false, lazy = false;  // lds_int, isplit
  bool fp_twin = false;     // isplit: the fp64 limbs' main step is k_split4_main_fp, which wants the key's fp64 twin built
  uint32_t fpmask = 0;      // isplit: data limbs on the fp64 kernels
};
inline ChunkRoute route_chunk(const RouteFacts &f, Seq seq, int nl, size_t cc) {
  ChunkRoute k;
  switch (seq) {
    case Seq::split14:
      // few ciphertexts in flight: the 139 KiB workgroups of the tensor kernel would leave most CUs idle for its whole
      // duration (measured at nl = 4: +5 % at 16 pairs, even at 32, -5 % at 48)
      k.lean = !f.sw.no_lean_front && cc * nl <= f.sw.lean_limit;
      // (measured at nl = 5 / 6 / 7, every prime below 2^50: +9.5 / -5 / -14 % against k_split3_main_fp: above five limbs the
      // prefetched key words push the kernel past 128 VGPRs and to one workgroup per CU)
      k.main4 = !f.sw.no_split4 && nl >= 1 && nl <= 5;
      k.pack = k.main4 && !f.sw.no_pack;
      break;
    case Seq::bsplit14: k.per_target = cc * nl < f.sw.pass0_target_limit; break;
    case Seq::lds_int:
      k.guard = f.guard;
      k.lazy = f.lazy;
      break;
    case Seq::isplit:
      k.guard = f.guard;
      k.fp_twin = f.logn == 14 && !f.sw.no_mixed;
      k.fpmask = (f.use_fp && !f.sw.no_mixed) ? f.fp_data_mask(nl) : 0u;
      break;
    default: break;
  }
  return k;
}

// ---- names, and a route as a short string, e.g. "split14 front=lean pack=1 main=split4" (tests and DESIGN.md quote these) ----
inline const char *name(Seq s) {
  constexpr const char *names[] = {"split14", "gsplit15", "isplit", "bsplit14", "bsplit_big", "lds_fp", "lds_int", "bmul", "generic"};
  return names[(int)s];
}
inline const char *name(KsFront k) { return k == KsFront::fp ? "fp" : k == KsFront::iks ? "iks" : "plain"; }
inline const char *name(BfvMul m) { return m == BfvMul::split ? "bmul" : m == BfvMul::big ? "bmul_big" : "behz"; }
inline const char *name(Rescale r) { return r == Rescale::fp ? "fp" : r == Rescale::mixed ? "mixed" : "generic"; }

// the key switch r of a call of `count` ciphertexts (per-chunk fields: its first chunk) into buf
inline void format_ks(char *buf, size_t cap, const RouteFacts &f, const KsRoute &r, int nl, size_t count) {
  const ChunkRoute k = route_chunk(f, r.seq, nl, plan_chunks(f, nl, count).chunk);
  switch (r.seq) {
    case Seq::split14: snprintf(buf, cap, "split14 front=%s pack=%d main=%s", k.lean ? "lean" : "fat", (int)k.pack, k.main4 ? "split4" : "split3"); break;
    case Seq::isplit: snprintf(buf, cap, "isplit%d guard=%d fpmask=0x%x", f.logn, (int)k.guard, (unsigned)k.fpmask); break;
    case Seq::bsplit14: snprintf(buf, cap, "bsplit14 pass0=%s", k.per_target ? "per_target" : "per_limb"); break;
    case Seq::lds_int: snprintf(buf, cap, "lds_int guard=%d lazy=%d", (int)k.guard, (int)k.lazy); break;
    case Seq::generic:
      if (r.front == KsFront::iks) snprintf(buf, cap, "generic front=iks guard=%d", (int)f.guard);
      else snprintf(buf, cap, "generic front=%s", name(r.front));
      break;
    default: snprintf(buf, cap, "%s", name(r.seq)); break;
  }
}
// The route of one call into buf: what abc_hip_route returns.  op: include/abc_hip.h, ABC_HIP_ROUTE_*.  Returns the length,
// -1 if cap is too small, -2 for an unknown op.
enum RouteOp { kRouteMulRelin = 0, kRouteKeyswitch = 1, kRouteRotate = 2, kRouteRescale = 3, kRouteMultiply = 4, kRouteRotateAdd = 5, kRouteRotateMacPlain = 7, kRouteMulPlainRescale = 10, kRouteMulSumRelin = 12 };  // 6, 8, 9 and 11 stay unassigned: the host tests probe them as unknown operations
inline int format_op(char *buf, size_t cap, const RouteFacts &f, int op, int nl, size_t count, bool in_place) {
  char ks[80];
  int n = -2;
  if (op == kRouteMulRelin) {
    const MulRoute r = route_mul_relin(f, nl);
    format_ks(ks, sizeof ks, f, r.seq == Seq::generic ? r.ks : KsRoute{r.seq, KsFront::plain}, nl, count);
    n = r.seq == Seq::generic ? snprintf(buf, cap, "generic mul=%s ks=%s", f.scheme == 2 ? "tensor" : name(r.mul), ks) : snprintf(buf, cap, "%s", ks);
  } else if (op == kRouteKeyswitch) {
    format_ks(ks, sizeof ks, f, route_keyswitch(f, nl), nl, count);
    n = snprintf(buf, cap, "%s", ks);
  } else if (op == kRouteRotate) {
    const RotRoute r = route_rotate(f, nl, in_place);
    format_ks(ks, sizeof ks, f, r.ks, nl, count);
    n = snprintf(buf, cap, "%s %s", r.fold ? "fold" : "permute", ks);
  } else if (op == kRouteRotateAdd) {
    const RotTailRoute r = route_rotate_add(f, nl, in_place);
    format_ks(ks, sizeof ks, f, r.rot.ks, nl, count);
    n = r.fused ? snprintf(buf, cap, "fold+add %s", ks) : snprintf(buf, cap, "%s add=separate %s", r.rot.fold ? "fold" : "permute", ks);
  } else if (op == kRouteRotateMacPlain) {
    const RotTailRoute r = route_rotate_mac(f, nl, in_place);
    format_ks(ks, sizeof ks, f, r.rot.ks, nl, count);
    n = r.fused ? snprintf(buf, cap, "fold+mac %s", ks) : snprintf(buf, cap, "%s mac=separate %s", r.rot.fold ? "fold" : "permute", ks);
  } else if (op == kRouteRescale) {
    const RescaleRoute r = route_rescale(f, nl, in_place);
    n = r.kind == Rescale::mixed ? snprintf(buf, cap, "mixed fpmask=0x%x", (unsigned)r.fpmask) : snprintf(buf, cap, "%s", name(r.kind));
  } else if (op == kRouteMulPlainRescale) {
    const MulPlainRescaleRoute r = route_mulplain_rescale(f, nl);
    const char *how = r.fused ? "fused" : "separate";
    n = r.rescale.kind == Rescale::mixed ? snprintf(buf, cap, "mixed fpmask=0x%x mulplain=%s", (unsigned)r.rescale.fpmask, how)
                                         : snprintf(buf, cap, "%s mulplain=%s", name(r.rescale.kind), how);
  } else if (op == kRouteMulSumRelin) {
    const MulSumRoute r = route_mul_sum(f, nl);
    format_ks(ks, sizeof ks, f, r.ks, nl, mul_sum_group(f, nl, count));  // per-chunk fields: those of the first group's first chunk
    n = snprintf(buf, cap, "%s tensor=%s", ks, r.sum ? "sum" : "per_term");
  } else if (op == kRouteMultiply) {
    n = snprintf(buf, cap, "%s", f.scheme == 1 ? name(route_bfv_multiply(f)) : "tensor");
  }
  return n < 0 ? n : (size_t)n < cap ? n : -1;
}
// ABC_HIP_ROUTE_DIAG_MATVEC_BSGS (13) has a formatter of its own, which abc_hip_route calls for that number: format_op keeps the
// set of operations it had (tests/cpp/test_route_mul_sum.cpp probes 13 there as an unknown operation).  The baby rotation's route,
// macsum=, the giant step's add=; returns the length, or -1 if cap is too small.
constexpr int kRouteDiagMatvecBsgs = 13;
inline int format_matvec_bsgs(char *buf, size_t cap, const RouteFacts &f, int nl, size_t count) {
  char ks[80];
  const MatvecBsgsRoute r = route_matvec_bsgs(f, nl);
  format_ks(ks, sizeof ks, f, r.baby.ks, nl, matvec_bsgs_group(f, nl, count, 1));  // per-chunk fields: those of the first group's first chunk
  const int n = snprintf(buf, cap, "%s %s macsum=%s add=%s", r.baby.fold ? "fold" : "permute", ks, r.macsum ? "kernel" : "per_term", r.giant.fused ? "fused" : "separate");
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}
// ABC_HIP_ROUTE_PLAIN_SUM_RESCALE (16) and ABC_HIP_ROUTE_DIAG_MATVEC_BSGS_RESCALE (17), formatters of their own like 13's.  16: the
// rescale's route, then sumrescale=fused|separate.  17: the baby rotation's route at nl, sumrescale=, then the giant step's route at
// nl - 1 with add=fused|separate; per-chunk fields: those of the first group's first chunk.  nl >= 2.  abc_hip_route has no argument
// for the number of terms: both strings answer for a sum of `count` size-2 ciphertexts of up to kPlainSumRescaleTerms terms (17: of
// the first group); a longer sum is separate unless ABC_HIP_PLAIN_SUM_RESCALE_TERMS is set.
constexpr int kRoutePlainSumRescale = 16, kRouteDiagMatvecBsgsRescale = 17;
inline int format_plain_sum_rescale(char *buf, size_t cap, const RouteFacts &f, int nl, size_t count) {
  const PlainSumRescaleRoute r = route_plain_sum_rescale(f, nl, count * 2, 1);
  const char *how = r.fused ? "fused" : "separate";
  const int n = r.rescale.kind == Rescale::mixed ? snprintf(buf, cap, "mixed fpmask=0x%x sumrescale=%s", (unsigned)r.rescale.fpmask, how)
                                                 : snprintf(buf, cap, "%s sumrescale=%s", name(r.rescale.kind), how);
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}
inline int format_matvec_bsgs_rescale(char *buf, size_t cap, const RouteFacts &f, int nl, size_t count) {
  char baby[80], giant[80];
  const size_t group = matvec_bsgs_group(f, nl, count, 1);
  const MatvecBsgsRescaleRoute r = route_matvec_bsgs_rescale(f, nl, group * 2, 1);
  format_ks(baby, sizeof baby, f, r.baby.ks, nl, group);
  format_ks(giant, sizeof giant, f, r.giant.rot.ks, nl - 1, group);
  const int n = snprintf(buf, cap, "%s %s sumrescale=%s %s %s add=%s", r.baby.fold ? "fold" : "permute", baby, r.sum.fused ? "fused" : "separate",
                         r.giant.rot.fold ? "fold" : "permute", giant, r.giant.fused ? "fused" : "separate");
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}
// ABC_HIP_ROUTE_CONST_SUM_RESCALE (18) and ABC_HIP_ROUTE_POLY_EVAL (19), formatters of their own like 13's.  18: the rescale's route at
// nl, then constsum=fused|separate for a sum of ONE term over `count` size-2 ciphertexts, every term at nl (abc_hip_route has no
// argument for the number of terms or their levels: more than kConstSumRescaleTerms terms, or a term above nl, is separate
// whatever the string says).  19: the mul_relin route at nl, then constsum=separate: from degree 2 on the last step reads powers held
// above its level (a degree-1 call follows string 18 at nl).
constexpr int kRouteConstSumRescale = 18, kRoutePolyEval = 19;
inline int format_const_sum_rescale(char *buf, size_t cap, const RouteFacts &f, int nl, size_t count) {
  const ConstSumRescaleRoute r = route_const_sum_rescale(f, nl, count * 2, 1, false);
  const char *how = r.fused ? "fused" : "separate";
  const int n = r.rescale.kind == Rescale::mixed ? snprintf(buf, cap, "mixed fpmask=0x%x constsum=%s", (unsigned)r.rescale.fpmask, how)
                                                 : snprintf(buf, cap, "%s constsum=%s", name(r.rescale.kind), how);
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}
inline int format_poly_eval(char *buf, size_t cap, const RouteFacts &f, int nl, size_t count) {
  char mul[128];
  if (format_op(mul, sizeof mul, f, kRouteMulRelin, nl, count, false) < 0) return -1;
  const int n = snprintf(buf, cap, "%s constsum=separate", mul);
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}
// ABC_HIP_ROUTE_BFV_PLAIN_SUM (14) and ABC_HIP_ROUTE_BFV_MATVEC_BSGS (15), formatters of their own for the same reason.  14:
// plainsum=fused / plainsum=ntt_domain for a call of `count` ciphertexts.  15: the baby rotation's route, the plainsum= of an inner
// sum over the first group, the giant step's add=; per-chunk fields and the group: those of a one-step baby list.
constexpr int kRouteBfvPlainSum = 14, kRouteBfvMatvecBsgs = 15;
inline const char *name(BfvPlainSum s) { return s == BfvPlainSum::fused ? "fused" : "ntt_domain"; }
inline int format_bfv_plain_sum(char *buf, size_t cap, const RouteFacts &f, size_t count) {
  const int n = snprintf(buf, cap, "plainsum=%s", name(route_bfv_plain_sum(f, count)));
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}
inline int format_bfv_matvec_bsgs(char *buf, size_t cap, const RouteFacts &f, size_t count) {
  char ks[80];
  const size_t group = matvec_bsgs_group(f, f.L, count, 1);
  const BfvMatvecBsgsRoute r = route_bfv_matvec_bsgs(f, group);
  format_ks(ks, sizeof ks, f, r.baby.ks, f.L, group);
  const int n = snprintf(buf, cap, "%s %s plainsum=%s add=%s", r.baby.fold ? "fold" : "permute", ks, name(r.sum), r.giant.fused ? "fused" : "separate");
  return n < 0 ? -1 : (size_t)n < cap ? n : -1;
}

}  // namespace abc
