// abc_context.hip -- context construction (device tables) and the extern "C" entry points of
// libabc_hip.so declared in include/abc_hip.h.
//
// abc_hip_ctx_create replaces SealCiphertextFactory::setupSealContext
// (src/runtime/SealCiphertextFactory.cpp:72-100): it fixes the modulus chain, builds the NTT twiddle
// tables (bit-reversed powers of the minimal primitive 2N-th root, with Shoup quotients), the BEHZ
// auxiliary bases {B, m_sk, gamma, m~ = 2^32} and every scalar constant the kernels need, and uploads
// them once; nothing is recomputed per operation.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../../include/abc_hip.h"
#include <dlfcn.h>

#include "abc_context.hpp"
#include "abc_host_math.hpp"
#include "abc_sample.hpp"

namespace abc {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

static bool env_on(const char *name) {  // set and not "0"
  const char *e = std::getenv(name);
  return e && !(e[0] == '0' && e[1] == 0);
}
void read_switches(abc_hip_ctx *c) {
  abc_hip_ctx::Switches s;
  s.no_fused = env_on("ABC_HIP_NO_FUSED");
  s.no_split = env_on("ABC_HIP_NO_SPLIT");
  s.no_split4 = env_on("ABC_HIP_NO_SPLIT4");
  s.no_isplit = env_on("ABC_HIP_NO_ISPLIT");
  s.no_gsplit = env_on("ABC_HIP_NO_GSPLIT");
  s.no_bsplit = env_on("ABC_HIP_NO_BSPLIT");
  s.no_mixed = env_on("ABC_HIP_NO_MIXED");
  s.no_pack = env_on("ABC_HIP_NO_PACK");
  s.no_key_twin = env_on("ABC_HIP_NO_KEY_TWIN");
  s.no_bmul = env_on("ABC_HIP_NO_BMUL");
  s.no_iks = env_on("ABC_HIP_NO_IKS");
  s.no_lean_front = env_on("ABC_HIP_NO_LEAN_FRONT");
  s.no_tensor_intt = env_on("ABC_HIP_NO_TENSOR_INTT");
  s.no_galois_fusion = env_on("ABC_HIP_NO_GALOIS_FUSION");
  s.no_rotate_add_fusion = env_on("ABC_HIP_NO_ROTATE_ADD_FUSION");
  s.no_rotate_mac_fusion = env_on("ABC_HIP_NO_ROTATE_MAC_FUSION");
  s.no_mulplain_rescale_fusion = env_on("ABC_HIP_NO_MULPLAIN_RESCALE_FUSION");
  s.no_tensor_sum = env_on("ABC_HIP_NO_TENSOR_SUM");
  s.no_plain_mac_sum = env_on("ABC_HIP_NO_PLAIN_MAC_SUM");
  s.no_plain_sum_rescale_fusion = env_on("ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION");
  s.no_const_mac_sum = env_on("ABC_HIP_NO_CONST_MAC_SUM");
  s.main_two_per_cu = env_on("ABC_HIP_MAIN_TWO_PER_CU");
  s.host_sampling = env_on("ABC_HIP_HOST_SAMPLING");
  if (const char *e = std::getenv("ABC_HIP_CHUNK")) s.chunk = (size_t)std::atol(e);
  if (const char *e = std::getenv("ABC_HIP_FEW_LIMBS")) s.few_limbs = (size_t)std::atol(e);
  if (const char *e = std::getenv("ABC_HIP_LEAN_LIMIT")) s.lean_limit = (size_t)std::atol(e);
  if (const char *e = std::getenv("ABC_HIP_PASS0_TARGET_LIMIT")) s.pass0_target_limit = (size_t)std::atol(e);
  if (const char *e = std::getenv("ABC_HIP_BFV_SCRATCH_MB")) s.bfv_scratch_mb = (size_t)std::atol(e);
  if (const char *e = std::getenv("ABC_HIP_PLAIN_SUM_RESCALE_TERMS")) s.plain_sum_rescale_terms = std::atoi(e);
  if (const char *e = std::getenv("ABC_HIP_CONST_SUM_RESCALE_FUSED")) s.const_sum_rescale_fused = std::atoi(e) ? 1 : 0;
  if (const char *e = std::getenv("ABC_HIP_LANES")) {
    s.lanes = std::atoi(e);
    if (s.lanes < 1) s.lanes = 1;
    if (s.lanes > abc_hip_ctx::kMaxLanes) s.lanes = abc_hip_ctx::kMaxLanes;
  }
  c->sw = s;
  // the facts the routes are a function of (abc_route.hpp): the primes are fixed by now, so this is the only walk over them
  RouteFacts &f = c->facts;
  f = RouteFacts{};
  f.scheme = c->scheme; f.logn = c->logn; f.K = c->K; f.L = c->L; f.nB = c->nB;
  f.use_fp = c->use_fp; f.behz_fp = c->behz_fp;
  f.big_block_log = big_block_log();
  for (int j = 0; j < c->K; j++) f.bits[j] = (unsigned char)c->h_mods[j].bits;
  f.sw = s;
  f.finish();
}

static Mod make_mod(uint64_t q, int logn, bool ntt) {
  using namespace host;
  Mod m{};
  m.q = q;
  m.two_q = 2 * q;
  const int k = bitlen(q);
  m.bits = (u32)k;
  m.shift = (u32)(k - 1);
  m.mu = (uint64_t)((((u128)1) << (k + 63)) / q);
  m.qd = (double)q;
  m.qinv = 1.0 / (double)q;
  if (ntt) {
    const uint64_t n = 1ull << logn;
    m.inv_n = invmod(n % q, q);
    m.inv_n_s = shoup(m.inv_n, q);
    if (fp_ok(m.bits)) {
      m.inv_n_c = m.inv_n > q / 2 ? -(double)(q - m.inv_n) : (double)m.inv_n;
      m.inv_n_cq = m.inv_n_c / m.qd;
    }
  }
  return m;
}

static void fill_twiddles(uint64_t q, int logn, uint64_t *dst /*[2][N][2]*/) {
  using namespace host;
  const size_t n = (size_t)1 << logn;
  const uint64_t psi = min_primitive_root(2 * n, q);
  uint64_t *fwd = dst, *inv = dst + 2 * n;  // interleaved {w, Shoup quotient}
  uint64_t p = 1;
  for (size_t i = 0; i < n; i++) {
    fwd[2 * (size_t)bitrev((uint32_t)i, logn)] = p;
    p = mulmod(p, psi, q);
  }
  const uint64_t ipsi = invmod(psi, q);
  p = 1;
  for (size_t i = 0; i < n; i++) {
    inv[2 * (size_t)bitrev((uint32_t)i, logn)] = p;
    p = mulmod(p, ipsi, q);
  }
  for (size_t i = 0; i < n; i++) {
    fwd[2 * i + 1] = shoup(fwd[2 * i], q);
    inv[2 * i + 1] = shoup(inv[2 * i], q);
  }
}

// fp64 twin of one modulus' twiddle table: w centred into (-q/2, q/2], one double per twiddle (exact: |w| < 2^49)
static void fill_fp_twiddles(uint64_t q, size_t n, const uint64_t *src /*[2][N][2]*/, double *dst /*[2][N]*/) {
  for (size_t i = 0; i < 2 * n; i++) {
    const uint64_t w = src[2 * i];
    dst[i] = w > q / 2 ? -(double)(q - w) : (double)w;
  }
}

static int build_context(abc_hip_ctx *c) {
  using namespace host;
  const int logn = c->logn, K = c->K, L = c->L;
  const size_t N = (size_t)c->n;
  const bool bfv = (c->scheme == ABC_HIP_SCHEME_BFV);
  std::vector<uint64_t> qs(c->primes.begin(), c->primes.begin() + L);
  const uint64_t qsp = c->primes[K - 1];
  DevConst &k = c->h_cst;
  std::memset(&k, 0, sizeof(k));

  // ---- modulus table ----
  c->mod_values.assign(c->primes.begin(), c->primes.end());
  std::vector<uint64_t> Bp;
  uint64_t m_sk = 0, gamma = 0;
  if (bfv) {
    // BEHZ auxiliary base, sized by SEAL's RNSTool rule.  SEAL draws m_sk, gamma and B from the 61-bit NTT primes.  The
    // q-residues a BFV multiply returns do not depend on which auxiliary primes carry the intermediate values (every
    // step computes residues of one fixed integer -- DESIGN.md section 4c; shown on the oracle by
    // tests/test_oracle_internal.py and on the device by every BFV parity test, whose oracle keeps SEAL's base), so where
    // every ciphertext prime is below 2^50 the base is drawn from the 50-bit primes instead: all BEHZ transforms then
    // take the exact-fp64 butterflies (8 instead of 16 instructions).  gamma (decryption only) stays SEAL's.
    bool fp_aux = !env_on("ABC_HIP_NO_FP64") && !env_on("ABC_HIP_BEHZ_SEAL_BASE");
    for (uint64_t q : c->primes) fp_aux = fp_aux && fp_ok((u32)bitlen(q));
    const int aux_bits = fp_aux ? 50 : 61;
    int nB = L;
    if (32 + bitlen(c->t) + prod_bitlen(qs) >= aux_bits * L + aux_bits) nB++;
    gamma = ntt_primes(N, 61, 2)[1];
    if (!fp_aux) {
      auto aux = ntt_primes(N, 61, (size_t)nB + 2);
      m_sk = aux[0];
      Bp.assign(aux.begin() + 2, aux.end());
    } else {
      std::vector<uint64_t> alt;
      for (uint64_t p : ntt_primes(N, 50, (size_t)nB + 1 + (size_t)K)) {
        bool clash = false;
        for (uint64_t q : c->primes) clash = clash || (p == q);
        if (!clash && alt.size() < (size_t)nB + 1) alt.push_back(p);
      }
      if (alt.size() < (size_t)nB + 1) throw std::runtime_error("not enough 50-bit NTT primes for the BEHZ auxiliary base");
      m_sk = alt[0];
      Bp.assign(alt.begin() + 1, alt.end());
    }
    // sums of up to L + 1 (resp. nB + 1) lazily reduced terms must stay below 2^53: 12 x 0.625 x 2^50
    c->behz_fp = fp_aux && L <= 10 && !env_on("ABC_HIP_BEHZ_INT_KERNELS");
    c->nB = nB;
    c->nBsk = nB + 1;
    for (uint64_t b : Bp) c->mod_values.push_back(b);
    c->mod_values.push_back(m_sk);
    c->mod_values.push_back(gamma);
    c->mod_values.push_back(c->t);
  }
  const int nmods = (int)c->mod_values.size();
  const int id_bsk = K, id_gamma = K + c->nBsk, id_t = K + c->nBsk + 1;
  c->h_mods.clear();
  std::vector<uint64_t> h_tw((size_t)nmods * 4 * N, 0);
  std::vector<double> h_ftw((size_t)nmods * 2 * N, 0.0);
  for (int i = 0; i < nmods; i++) {
    const bool ntt = !(bfv && i == id_gamma);
    c->h_mods.push_back(make_mod(c->mod_values[i], logn, ntt));
    if (ntt) fill_twiddles(c->mod_values[i], logn, h_tw.data() + (size_t)i * 4 * N);
    if (ntt && fp_ok(c->h_mods.back().bits))
      fill_fp_twiddles(c->mod_values[i], N, h_tw.data() + (size_t)i * 4 * N, h_ftw.data() + (size_t)i * 2 * N);
  }

  // ---- key / modulus switching constants ----
  for (int j = 0; j < L; j++) {
    const uint64_t q = qs[j];
    k.inv_special[j] = invmod(qsp % q, q);
    k.inv_special_s[j] = shoup(k.inv_special[j], q);
    k.special_mod_q[j] = qsp % q;
    k.special_mod_q_s[j] = shoup(k.special_mod_q[j], q);
    k.inv_special_c[j] = k.inv_special[j] > q / 2 ? -(double)(q - k.inv_special[j]) : (double)k.inv_special[j];
    k.inv_special_cq[j] = k.inv_special_c[j] / (double)q;
    k.special_c[j] = k.special_mod_q[j] > q / 2 ? -(double)(q - k.special_mod_q[j]) : (double)k.special_mod_q[j];
    k.special_cq[j] = k.special_c[j] / (double)q;
  }
  for (int l = 1; l < L; l++)
    for (int j = 0; j < l; j++) {
      k.inv_qlast[l][j] = invmod(qs[l] % qs[j], qs[j]);
      k.inv_qlast_s[l][j] = shoup(k.inv_qlast[l][j], qs[j]);
      k.inv_qlast_c[l][j] = k.inv_qlast[l][j] > qs[j] / 2 ? -(double)(qs[j] - k.inv_qlast[l][j]) : (double)k.inv_qlast[l][j];
      k.inv_qlast_cq[l][j] = k.inv_qlast_c[l][j] / (double)qs[j];
    }

  std::vector<uint32_t> slot_map;
  if (bfv) {
    const uint64_t t = c->t;
    k.t = t;
    k.q_mod_t = prod_mod(qs, t);
    k.upper_half_threshold = (t + 1) >> 1;
    for (int i = 0; i < L; i++) {
      const uint64_t q = qs[i];
      // floor(Q/t) mod q_i = -(Q mod t) * t^-1 mod q_i
      k.coeff_div_plain[i] = mulmod(negmod(k.q_mod_t, q), invmod(t % q, q), q);
      k.upper_half_increment[i] = q - t;
    }
    // BatchEncoder slot -> coefficient-index map: slot i of row 0 <-> evaluation at psi^(3^i)
    slot_map.resize(N);
    const size_t row = N >> 1, m = N << 1;
    uint64_t pos = 1;
    for (size_t i = 0; i < row; i++) {
      slot_map[i] = bitrev((uint32_t)((pos - 1) >> 1), logn);
      slot_map[row | i] = bitrev((uint32_t)((m - pos - 1) >> 1), logn);
      pos = (pos * 3) & (m - 1);
    }
    // ---- BEHZ ----
    const int nB = c->nB, nBsk = c->nBsk;
    const uint64_t mt = 1ull << 32;
    std::vector<uint64_t> bsk(Bp);
    bsk.push_back(m_sk);
    k.nq = L; k.nB = nB; k.nBsk = nBsk;
    auto punct_mod = [&](const std::vector<uint64_t> &base, int skip, uint64_t p) {
      uint64_t v = 1 % p;
      for (int i = 0; i < (int)base.size(); i++)
        if (i != skip) v = mulmod(v, base[i] % p, p);
      return v;
    };
    for (int i = 0; i < L; i++) {
      const uint64_t q = qs[i];
      k.mtilde_mod_q[i] = mt % q;
      k.inv_punct_q[i] = invmod(punct_mod(qs, i, q), q);
      for (int j = 0; j < nBsk; j++) {
        k.q_to_bsk[j][i] = punct_mod(qs, i, bsk[j]);
        k.q_to_bsk_s[j][i] = shoup(k.q_to_bsk[j][i], bsk[j]);
      }
      k.q_to_mtilde[i] = punct_mod(qs, i, mt);
      k.q_to_t[i] = punct_mod(qs, i, t);
      k.q_to_gamma[i] = punct_mod(qs, i, gamma);
      k.B_mod_q[i] = prod_mod(Bp, q);
      k.t_mod_q[i] = t % q;
      k.tgamma_mod_q[i] = mulmod(t % q, gamma % q, q);
      for (int b = 0; b < nB; b++) {
        k.B_to_q[i][b] = punct_mod(Bp, b, q);
        k.B_to_q_s[i][b] = shoup(k.B_to_q[i][b], q);
      }
    }
    k.neg_inv_q_mod_mtilde = negmod(invmod(prod_mod(qs, mt), mt), mt);
    for (int j = 0; j < nBsk; j++) {
      const uint64_t p = bsk[j];
      k.q_mod_bsk[j] = prod_mod(qs, p);
      k.q_mod_bsk_s[j] = shoup(k.q_mod_bsk[j], p);
      k.inv_q_mod_bsk[j] = invmod(k.q_mod_bsk[j], p);
      k.inv_mtilde_mod_bsk[j] = invmod(mt % p, p);
      k.t_mod_bsk[j] = t % p;
    }
    for (int b = 0; b < nB; b++) {
      k.inv_punct_B[b] = invmod(punct_mod(Bp, b, Bp[b]), Bp[b]);
      k.B_to_msk[b] = punct_mod(Bp, b, m_sk);
      k.B_to_msk_s[b] = shoup(k.B_to_msk[b], m_sk);
    }
    k.inv_B_mod_msk = invmod(prod_mod(Bp, m_sk), m_sk);
    k.inv_B_mod_msk_s = shoup(k.inv_B_mod_msk, m_sk);
    for (int i = 0; i < L; i++) {
      const uint64_t q = qs[i];
      k.ext_q[i] = mulmod(k.mtilde_mod_q[i], k.inv_punct_q[i], q);
      k.ext_q_s[i] = shoup(k.ext_q[i], q);
      k.flr_q[i] = mulmod(k.t_mod_q[i], k.inv_punct_q[i], q);
      k.flr_q_s[i] = shoup(k.flr_q[i], q);
      k.dec_q[i] = mulmod(k.tgamma_mod_q[i], k.inv_punct_q[i], q);
      k.dec_q_s[i] = shoup(k.dec_q[i], q);
      k.B_mod_q_s[i] = shoup(k.B_mod_q[i], q);
    }
    for (int j = 0; j < nBsk; j++) {
      const uint64_t p = bsk[j];
      k.tinvq_bsk[j] = mulmod(k.t_mod_bsk[j], k.inv_q_mod_bsk[j], p);
      k.tinvq_bsk_s[j] = shoup(k.tinvq_bsk[j], p);
      k.inv_q_mod_bsk_s[j] = shoup(k.inv_q_mod_bsk[j], p);
      k.inv_mtilde_mod_bsk_s[j] = shoup(k.inv_mtilde_mod_bsk[j], p);
    }
    for (int b = 0; b < nB; b++) k.inv_punct_B_s[b] = shoup(k.inv_punct_B[b], Bp[b]);
    k.neg_inv_q_mod_t = negmod(invmod(prod_mod(qs, t), t), t);
    k.neg_inv_q_mod_gamma = negmod(invmod(prod_mod(qs, gamma), gamma), gamma);
    k.inv_gamma_mod_t = invmod(gamma % t, t);
    k.gamma = gamma;
  }

  // ---- upload ----
  ABC_HIP_CHECK(hipMalloc(&c->d_mods, nmods * sizeof(Mod)));
  ABC_HIP_CHECK(hipMemcpy(c->d_mods, c->h_mods.data(), nmods * sizeof(Mod), hipMemcpyHostToDevice));
  ABC_HIP_CHECK(hipMalloc(&c->d_tw, h_tw.size() * 8));
  ABC_HIP_CHECK(hipMemcpy(c->d_tw, h_tw.data(), h_tw.size() * 8, hipMemcpyHostToDevice));
  ABC_HIP_CHECK(hipMalloc(&c->d_ftw, h_ftw.size() * 8));
  ABC_HIP_CHECK(hipMemcpy(c->d_ftw, h_ftw.data(), h_ftw.size() * 8, hipMemcpyHostToDevice));
  c->use_fp = !env_on("ABC_HIP_NO_FP64");
  read_switches(c);  // after the moduli: the route facts hold their widths
  ABC_HIP_CHECK(hipMalloc(&c->d_cst, sizeof(DevConst)));
  ABC_HIP_CHECK(hipMemcpy(c->d_cst, &k, sizeof(DevConst), hipMemcpyHostToDevice));
  if (bfv && c->behz_fp) {
    // {centred value, value / p} pairs of every BEHZ constant
    auto pair = [](double (&dst)[2], uint64_t v, uint64_t p) {
      const double vc = v > p / 2 ? -(double)(p - v) : (double)v;
      dst[0] = vc;
      dst[1] = vc / (double)p;
    };
    std::vector<DevConstFp> hf(1);
    DevConstFp &f = hf[0];
    std::memset(&f, 0, sizeof(f));
    const int nB = c->nB, nBsk = c->nBsk;
    std::vector<uint64_t> bskv(Bp);
    bskv.push_back(m_sk);
    for (int i = 0; i < L; i++) {
      pair(f.ext_q[i], k.ext_q[i], qs[i]);
      pair(f.flr_q[i], k.flr_q[i], qs[i]);
      pair(f.B_mod_q[i], k.B_mod_q[i], qs[i]);
      for (int b = 0; b < nB; b++) pair(f.B_to_q[i][b], k.B_to_q[i][b], qs[i]);
    }
    for (int j = 0; j < nBsk; j++) {
      for (int i = 0; i < L; i++) pair(f.q_to_bsk[j][i], k.q_to_bsk[j][i], bskv[j]);
      pair(f.q_mod_bsk[j], k.q_mod_bsk[j], bskv[j]);
      pair(f.inv_mtilde_mod_bsk[j], k.inv_mtilde_mod_bsk[j], bskv[j]);
      pair(f.tinvq_bsk[j], k.tinvq_bsk[j], bskv[j]);
      pair(f.inv_q_mod_bsk[j], k.inv_q_mod_bsk[j], bskv[j]);
    }
    for (int b = 0; b < nB; b++) {
      pair(f.inv_punct_B[b], k.inv_punct_B[b], Bp[b]);
      pair(f.B_to_msk[b], k.B_to_msk[b], m_sk);
    }
    pair(f.inv_B_mod_msk, k.inv_B_mod_msk, m_sk);
    ABC_HIP_CHECK(hipMalloc(&c->d_cstf, sizeof(DevConstFp)));
    ABC_HIP_CHECK(hipMemcpy(c->d_cstf, &f, sizeof(DevConstFp), hipMemcpyHostToDevice));
  }
  if (bfv) {
    ABC_HIP_CHECK(hipMalloc(&c->d_slot_map, N * 4));
    ABC_HIP_CHECK(hipMemcpy(c->d_slot_map, slot_map.data(), N * 4, hipMemcpyHostToDevice));
  }
  DevCtx &dc = c->dc;
  dc.mods = c->d_mods; dc.tw = c->d_tw; dc.ftw = c->d_ftw; dc.cst = c->d_cst; dc.cstf = c->d_cstf; dc.slot_map = c->d_slot_map;
  dc.logn = logn; dc.n = (int)N; dc.K = K; dc.L = L;
  dc.ps = (int)N;
  dc.id_bsk = id_bsk; dc.id_t = id_t; dc.id_gamma = id_gamma; dc.id_mtilde = -1;
  return 0;
}

// ---- rotation bookkeeping (GaloisTool::get_elt_from_step, util::naf) ----
static uint32_t elt_from_step(const abc_hip_ctx *c, int step) {
  const uint32_t n = (uint32_t)c->n;
  const uint64_t m = 2ull * n;
  if (step == 0) return (uint32_t)(m - 1);
  const bool neg = step < 0;
  const uint32_t pos = (uint32_t)(neg ? -step : step);
  if (pos >= (n >> 1)) return 0;
  const int s = neg ? (int)(n >> 1) - (int)pos : (int)pos;
  uint64_t g = 1;
  for (int i = 0; i < s; i++) g = (g * 3) & (m - 1);
  return (uint32_t)g;
}

static std::vector<int> naf(int value) {
  std::vector<int> out;
  const bool sign = value < 0;
  value = std::abs(value);
  for (int i = 0; value; i++) {
    const int zi = (value & 1) ? 2 - (value & 3) : 0;
    value = (value - zi) >> 1;
    if (zi) out.push_back((sign ? -zi : zi) * (1 << i));
  }
  return out;
}

// the record of a key switch over whole ciphertexts at `ct`, `size` polynomials each: the last one is switched, (c0, c1) -- c0 alone
// at size 2 -- is the addend
static KsOperands ks_of_ciphertexts(const abc_hip_ctx *c, const u64 *ct, int size, const u64 *key, u64 *out, int nl, size_t count) {
  const size_t pw = (size_t)nl * c->n;
  KsOperands o;
  o.target = ct + (size - 1) * pw, o.addend = ct, o.target_stride = o.addend_stride = size * pw, o.add_c1 = size == 3;
  o.key = key, o.out = out, o.nl = nl, o.count = count;
  return o;
}

// a [a, a + a_bytes) and b [b, b + b_bytes) share a byte
static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// one Galois element along route r; tail (a fused route only): the key switch's last kernel adds tail.addend, or multiplies by
// tail.plain and then adds tail.addend where there is one
static int apply_galois_routed(abc_hip_ctx *c, const RotRoute &r, const u64 *in, u64 *out, int nl, uint32_t elt, size_t count,
                               const RotTail &tail = {}) {
  auto it = c->d_galois.find(elt);
  if (it == c->d_galois.end()) { set_error("Galois key not present"); return 1; }
  if (!count) return 0;
  // out = (g(c0) + ks0, ks1) with ks = KeySwitch(g(c1)); r.fold: the permutation is a gather inside the key-switch kernels
  if (!r.fold) {  // g(c0), g(c1) live in arena 0 (keyswitch_generic uses c->ws)
    if (ensure_aux(c, 0, count * 2 * (size_t)nl * c->n * 8)) return 1;
    if (launch_galois(c, in, (u64 *)c->aux[0], nl, count * 2, elt, c->scheme == ABC_HIP_SCHEME_CKKS)) return 1;
    in = (const u64 *)c->aux[0];
  }
  KsOperands o = ks_of_ciphertexts(c, in, 2, it->second, out, nl, count);
  o.gelt = r.fold ? elt : 0u;
  o.acc = tail.addend, o.plain = tail.plain, o.plain_stride = tail.plain_stride;
  return launch_keyswitch(c, r.ks, o);
}

// out = tail applied to a ciphertext x that `out` is or does not overlap (step 0's input, or a rotation in an arena), as separate kernels:
// the product with the plaintext -- into `out` without an addend, else in place on x where it is scratch (x_scratch), else in
// arena `tmp_arena` -- then the add kernel (elementwise, so every aliasing of its three pointers is fine); a copy for an empty tail
static int finish_separate(abc_hip_ctx *c, u64 *x_scratch, const u64 *x, const RotTail &tail, u64 *out, int nl, size_t count, int tmp_arena) {
  const size_t bytes = count * 2 * nl * (size_t)c->n * 8;
  if (tail.plain) {
    if (!tail.addend) return ckks_multiply_plain(c, x, tail.plain, tail.plain_stride, out, 2, nl, count);
    if (!x_scratch) {
      if (ensure_aux(c, tmp_arena, bytes)) return 1;
      x_scratch = (u64 *)c->aux[tmp_arena];
    }
    if (ckks_multiply_plain(c, x, tail.plain, tail.plain_stride, x_scratch, 2, nl, count)) return 1;
    x = x_scratch;
  }
  if (tail.addend) return launch_addsub(c, tail.addend, x, out, nl, count * 2, 0);
  if (x != out) ABC_HIP_CHECK(hipMemcpyAsync(out, x, bytes, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// out = tail applied to g(in): every abc_hip_apply_galois* entry, and each hop of rotate_tail.  Fused: the tail's operands go to
// the key switch's last kernel; `out` may be the addend there, and is never `in`.  A plain rotation is "fused" whenever it is out
// of place.  Otherwise the rotation lands in arena `tmp_arena` -- never in place, whatever `out` is -- and finish_separate follows.
static int apply_galois_tail(abc_hip_ctx *c, const u64 *in, const RotTail &tail, u64 *out, int nl, uint32_t elt, size_t count, int tmp_arena) {
  if (!c->d_galois.count(elt)) { set_error("Galois key not present"); return 1; }
  if (!count) return 0;
  const RotTailRoute r = tail.plain    ? route_rotate_mac(c->facts, nl, in == out)
                         : tail.addend ? route_rotate_add(c->facts, nl, in == out)
                                       : RotTailRoute{route_rotate(c->facts, nl, false), in != out};
  if (r.fused) return apply_galois_routed(c, r.rot, in, out, nl, elt, count, tail);
  if (ensure_aux(c, tmp_arena, count * 2 * nl * (size_t)c->n * 8)) return 1;
  u64 *tmp = (u64 *)c->aux[tmp_arena];
  if (apply_galois_routed(c, r.rot, in, tmp, nl, elt, count)) return 1;
  return finish_separate(c, tmp, tmp, tail, out, nl, count, tmp_arena);
}

// the hops of one rotation: the step itself where it has a key, else its non-adjacent form; fails before anything is launched
static int rotation_terms(abc_hip_ctx *c, int steps, std::vector<int> &terms) {
  const uint32_t elt = elt_from_step(c, steps);
  if (!elt) { set_error("step count too large"); return 1; }
  if (c->d_galois.count(elt)) {
    terms.push_back(steps);
  } else {
    // no key for this element: SEAL decomposes the step count in non-adjacent form (Evaluator::rotate_internal)
    for (int s : naf(steps))
      if ((size_t)std::abs(s) != ((size_t)c->n >> 1)) terms.push_back(s);
    if (naf(steps).size() == 1) { set_error("Galois key not present"); return 1; }
    for (int s : terms)
      if (!c->d_galois.count(elt_from_step(c, s))) { set_error("Galois key not present"); return 1; }
  }
  return 0;
}

// every step of a list and every key it needs, before the first launch of the call
static int check_steps(abc_hip_ctx *c, const std::vector<int> &steps) {
  for (int s : steps) {
    std::vector<int> terms;
    if (s && rotation_terms(c, s, terms)) return 1;
  }
  return 0;
}

// out = tail applied to rotate(in, steps): abc_hip_rotate (empty tail), abc_hip_rotate_add, abc_hip_rotate_mac_plain.  Step 0 has no
// key switch (a plaintext with an addend multiplies into arena 1).  Hop i of the chain lands in arena 1 + (i & 1) (every hop is out
// of place); the last one takes the tail and lands in `out`, with the arena the ping-pong would use next as its temporary where
// its route does not fuse -- a plain rotation in place included, which is that hop into the arena and a copy.
static int rotate_tail(abc_hip_ctx *c, const u64 *in, const RotTail &tail, u64 *out, int nl, int steps, size_t count) {
  if (steps == 0) return count ? finish_separate(c, nullptr, in, tail, out, nl, count, 1) : 0;
  std::vector<int> terms;
  if (rotation_terms(c, steps, terms)) return 1;
  if (!count) return 0;
  const u64 *cur = in;
  const size_t last = terms.size() - 1;
  for (size_t i = 0; i < last; i++) {
    const int which = 1 + (int)(i & 1);
    if (ensure_aux(c, which, count * 2 * nl * (size_t)c->n * 8)) return 1;
    u64 *dst = (u64 *)c->aux[which];
    if (apply_galois_tail(c, cur, {}, dst, nl, elt_from_step(c, terms[i]), count, which)) return 1;
    cur = dst;
  }
  return apply_galois_tail(c, cur, tail, out, nl, elt_from_step(c, terms[last]), count, 1 + (int)(last & 1));
}

// out = sum_r diags[r] (.) rotate(in, steps[r]), in the order given: the running sum lives in `out`, every term after the first is
// one rotate_tail with out as its addend
static int diag_matvec(abc_hip_ctx *c, const u64 *in, const u64 *diags, size_t diag_stride, const std::vector<int> &steps, u64 *out, int nl,
                       size_t count) {
  const size_t bytes = count * 2 * (size_t)nl * c->n * 8;
  if (check_steps(c, steps)) return 1;
  if (!count) return 0;
  if (ranges_overlap(in, bytes, out, bytes)) { set_error("diag_matvec: d_out must not overlap d_in"); return 1; }
  if (steps.empty()) {
    ABC_HIP_CHECK(hipMemsetAsync(out, 0, bytes, c->stream));
    return 0;
  }
  for (size_t r = 0; r < steps.size(); r++)
    if (rotate_tail(c, in, {r ? out : nullptr, diags + r * diag_stride, 0}, out, nl, steps[r], count)) return 1;
  return 0;
}

// acc = in; acc = acc + rotate(acc, s) for each step in order; out = acc.  The running sums ping-pong through arenas 3 and 4
// (0 .. 2 belong to the rotations), only the last one lands in `out`, which may therefore be `in`.
static int rotate_sum(abc_hip_ctx *c, const u64 *in, u64 *out, int nl, const std::vector<int> &steps, size_t count) {
  if (check_steps(c, steps)) return 1;
  if (!count) return 0;
  const size_t bytes = count * 2 * nl * (size_t)c->n * 8;
  if (steps.empty()) {
    if (in != out) ABC_HIP_CHECK(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  if (steps.size() > 1 && (ensure_aux(c, 3, bytes) || (steps.size() > 2 && ensure_aux(c, 4, bytes)))) return 1;
  const u64 *acc = in;
  for (size_t i = 0; i < steps.size(); i++) {
    u64 *dst = (i + 1 == steps.size()) ? out : (u64 *)c->aux[3 + (i & 1)];
    if (rotate_tail(c, acc, {acc}, dst, nl, steps[i], count)) return 1;
    acc = dst;
  }
  return 0;
}

// Several Galois elements of one input, out[r] = (g(ks0 + c0), g(ks1)) with ks = KeySwitch(c1, key'_g) on the UNPERMUTED c1
// (DESIGN.md section 4).  elts[r] == 0: slab r is a copy of the input (rotate_hoisted's step 0).  Every argument is checked before
// anything is launched; the permuted keys are built next (mirrors of keys: a later failure leaves them, as a first use of a key's
// fp64 twin would), and the arena grows last, so a call that fails has written no ciphertext and no scratch.  Per element the key
// switch is the plain one of this level (route_keyswitch): nothing is shared between the elements yet.
static int hoisted(abc_hip_ctx *c, const u64 *in, u64 *out, int nl, const std::vector<uint32_t> &elts, size_t count) {
  const size_t N = (size_t)c->n, pw = (size_t)nl * N, ctw = count * 2 * pw;
  const uint64_t m = 2 * (uint64_t)N;
  std::vector<const u64 *> keys(elts.size(), nullptr);
  for (size_t r = 0; r < elts.size(); r++) {
    if (!elts[r]) continue;
    auto it = c->d_galois.find(elts[r]);
    if (it == c->d_galois.end()) { set_error("Galois key not present"); return 1; }
    keys[r] = it->second;
  }
  if (elts.empty() || !count) return 0;
  if (ranges_overlap(in, ctw * 8, out, elts.size() * ctw * 8)) { set_error("hoisted rotations: d_out must not overlap d_in"); return 1; }
  for (size_t r = 0; r < elts.size(); r++)  // inside a capture they must exist already
    if (keys[r] && !(keys[r] = key_permuted(c, keys[r], (uint32_t)host::invmod(elts[r], m)))) return 1;
  if (ensure_aux(c, 0, ctw * 8)) return 1;
  const bool ntt_form = (c->scheme == ABC_HIP_SCHEME_CKKS);
  u64 *ks = (u64 *)c->aux[0];
  for (size_t r = 0; r < elts.size(); r++) {
    u64 *slab = out + r * ctw;
    if (!elts[r]) {
      ABC_HIP_CHECK(hipMemcpyAsync(slab, in, ctw * 8, hipMemcpyDeviceToDevice, c->stream));
      continue;
    }
    if (launch_keyswitch(c, route_keyswitch(c->facts, nl), ks_of_ciphertexts(c, in, 2, keys[r], ks, nl, count))) return 1;
    if (launch_galois(c, ks, slab, nl, count * 2, elts[r], ntt_form)) return 1;
  }
  return 0;
}

static int relinearize(abc_hip_ctx *c, const u64 *ct3, u64 *out2, int nl, size_t count) {
  if (!c->d_relin) { set_error("relinearize: no relinearisation key"); return 1; }
  // target = c2 (poly 2 of each size-3 ciphertext); addend = (c0, c1)
  return launch_keyswitch(c, route_keyswitch(c->facts, nl), ks_of_ciphertexts(c, ct3, 3, c->d_relin, out2, nl, count));
}

// out = sum over k of a[k] (x) b[k], size 3 (relin false: out is [count][3][nl][N]) or relinearised (out [count][2][nl][N]).  The
// caller has checked the level, the pointers, the overlaps and the key.  The batch goes in groups of ciphertexts (mul_sum_group):
// per group the size-3 sum is formed -- in place in `out`, or in arena 1 where the key switch follows -- by the K-term kernel, or,
// on the per-term route, product by product through arena 2 and the add kernel; then the group's key switch writes its slice of
// `out`.  A term that IS `out` (relin only) is therefore read by its own group before that group's slice is written, and by no other.
static int mul_sum(abc_hip_ctx *c, const std::vector<const u64 *> &a, const std::vector<const u64 *> &b, u64 *out, bool relin, int nl,
                   size_t count) {
  if (!count) return 0;
  const size_t pw = (size_t)nl * c->n, K = a.size();
  if (!K) {
    ABC_HIP_CHECK(hipMemsetAsync(out, 0, count * (relin ? 2 : 3) * pw * 8, c->stream));
    return 0;
  }
  const MulSumRoute r = route_mul_sum(c->facts, nl);
  const size_t group = mul_sum_group(c->facts, nl, count);
  if (relin && ensure_aux(c, 1, group * 3 * pw * 8)) return 1;
  if (!r.sum && K > 1 && ensure_aux(c, 2, group * 3 * pw * 8)) return 1;
  std::vector<const u64 *> ga(K), gb(K);
  for (size_t off = 0; off < count; off += group) {
    const size_t cc = count - off < group ? count - off : group;
    u64 *sum3 = relin ? (u64 *)c->aux[1] : out + off * 3 * pw;
    for (size_t k = 0; k < K; k++) ga[k] = a[k] + off * 2 * pw, gb[k] = b[k] + off * 2 * pw;
    if (r.sum) {
      if (launch_ckks_tensor_sum(c, ga.data(), gb.data(), (int)K, sum3, nl, cc)) return 1;
    } else {
      for (size_t k = 0; k < K; k++) {
        u64 *dst = k ? (u64 *)c->aux[2] : sum3;
        if (c->scheme == ABC_HIP_SCHEME_CKKS ? launch_ckks_tensor(c, ga[k], gb[k], dst, nl, cc) : bfv_multiply(c, route_bfv_multiply(c->facts), ga[k], gb[k], dst, cc)) return 1;
        if (k && launch_addsub(c, sum3, dst, sum3, nl, cc * 3, 0)) return 1;
      }
    }
    if (relin && launch_keyswitch(c, r.ks, ks_of_ciphertexts(c, sum3, 3, c->d_relin, out + off * 2 * pw, nl, cc))) return 1;
  }
  return 0;
}

// out = (addend or 0) + sum over k of plain[k] (.) ct[k], [count][size][nl][N] (CKKS); out may BE addend and overlaps nothing else
// (the caller has checked).  One K-term kernel, or -- kernel false -- term by term: the product lands in `out` where nothing is
// carried yet, else in arena 2 (idle between two rotations), and the add kernel follows.
static int plain_mac_sum(abc_hip_ctx *c, bool kernel, const std::vector<const u64 *> &ct, const std::vector<const u64 *> &plain, size_t plain_stride,
                         const u64 *addend, u64 *out, int size, int nl, size_t count) {
  if (!count) return 0;
  const size_t bytes = count * size * (size_t)nl * c->n * 8;
  if (ct.empty()) {
    if (!addend) ABC_HIP_CHECK(hipMemsetAsync(out, 0, bytes, c->stream));
    else if (addend != out) ABC_HIP_CHECK(hipMemcpyAsync(out, addend, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  if (kernel) return launch_ckks_plain_mac_sum(c, ct.data(), plain.data(), plain_stride, (int)ct.size(), addend, out, size, nl, count);
  if ((addend || ct.size() > 1) && ensure_aux(c, 2, bytes)) return 1;
  const u64 *carry = addend;
  for (size_t k = 0; k < ct.size(); k++) {
    u64 *dst = carry ? (u64 *)c->aux[2] : out;
    if (ckks_multiply_plain(c, ct[k], plain[k], plain_stride, dst, size, nl, count)) return 1;
    if (carry && launch_addsub(c, carry, dst, out, nl, count * size, 0)) return 1;
    carry = out;
  }
  return 0;
}

// out [count][size][nl-1][N] = rescale((addend or 0) + sum over k of plain[k] (.) ct[k]) (CKKS, nl >= 2); out overlaps no operand (the
// caller has checked).  Fused (route_plain_sum_rescale: by measurement sums of up to four terms on large batches, every term in the
// pair; under ABC_HIP_PLAIN_SUM_RESCALE_TERMS every sum): the terms the fused pair does not take (plain_sum_rescale_lead) are summed
// into arena 1 by plain_mac_sum with the addend as their first carry, and the pair takes the rest with that arena (or the addend) as
// its carry.  Separate: the whole sum into arena 1, then launch_rescale.  Arena 2 is plain_mac_sum's on its per-term route.
static int plain_sum_rescale(abc_hip_ctx *c, const std::vector<const u64 *> &ct, const std::vector<const u64 *> &plain, size_t plain_stride,
                             const u64 *addend, u64 *out, int size, int nl, size_t count) {
  if (!count) return 0;
  const size_t N = (size_t)c->n, in_bytes = count * size * (size_t)nl * N * 8;
  const int K = (int)ct.size();
  if (!K && !addend) {  // rescale(0) = 0
    ABC_HIP_CHECK(hipMemsetAsync(out, 0, count * size * (size_t)(nl - 1) * N * 8, c->stream));
    return 0;
  }
  if (!K) return launch_rescale(c, addend, out, size, nl, count);
  const PlainSumRescaleRoute r = route_plain_sum_rescale(c->facts, nl, count * size, K);
  const int lead = r.fused ? plain_sum_rescale_lead(K, r.fused_terms) : K;
  const u64 *carry = addend;
  if (lead) {
    if (ensure_aux(c, 1, in_bytes)) return 1;
    u64 *sum = (u64 *)c->aux[1];
    if (plain_mac_sum(c, route_plain_mac_sum(c->facts, nl), std::vector<const u64 *>(ct.begin(), ct.begin() + lead),
                      std::vector<const u64 *>(plain.begin(), plain.begin() + lead), plain_stride, addend, sum, size, nl, count))
      return 1;
    carry = sum;
  }
  if (!r.fused) return launch_rescale(c, carry, out, size, nl, count);
  return launch_plain_sum_rescale(c, r.rescale, ct.data() + lead, plain.data() + lead, plain_stride, K - lead, carry, out, size, nl, count);
}

// value * scale, rounded to the nearest integer (ties away from zero), modulo the first nl data primes: the words of the constant
// `value` at `scale` in NTT form (every word of limb j is w[j]).  |r| < 2^62 is the encoder's own limit.  No GPU work.
static int const_words(abc_hip_ctx *c, const char *op, double value, double scale, int nl, u64 *w) {
  const double r = std::round(value * scale);
  if (!std::isfinite(r)) { set_error(std::string(op) + ": value * scale is not finite"); return 1; }
  if (std::fabs(r) >= 4611686018427387904.0) { set_error(std::string(op) + ": |value * scale| must stay below 2^62"); return 1; }
  const long long ri = (long long)r;
  const u64 mag = ri < 0 ? (u64)(-ri) : (u64)ri;
  for (int j = 0; j < nl; j++) {
    const u64 q = c->primes[j], m = mag % q;
    w[j] = (ri < 0 && m) ? q - m : m;
  }
  return 0;
}

// out [count][size][nl][N] = (addend or 0) + cst (component 0) + sum over k of w[k] * ct[k] (CKKS); term k is [count][size][ct_nl[k]][N],
// ct_nl[k] >= nl; w: [K][nl] words, cst: [nl] words or null; out may BE addend and overlaps nothing else (the caller has checked).
// One K-term kernel, or -- kernel false -- the sequence a caller composes: per term the first nl limbs copied out where the term is
// held higher (mod_switch; arena 6 behind the constant plaintext), the weight filled into a plaintext (arena 6), multiply_plain --
// into `out` where nothing is carried yet, else into arena 2 and the add kernel -- and last add_plain of the filled constant.
static int const_mac_sum(abc_hip_ctx *c, bool kernel, const std::vector<const u64 *> &ct, const std::vector<int> &ct_nl, const u64 *w, const u64 *cst,
                         const u64 *addend, u64 *out, int size, int nl, size_t count) {
  if (!count) return 0;
  const size_t pw = (size_t)nl * c->n, words = count * size * pw, bytes = words * 8;
  if (ct.empty() && !cst) {
    if (!addend) ABC_HIP_CHECK(hipMemsetAsync(out, 0, bytes, c->stream));
    else if (addend != out) ABC_HIP_CHECK(hipMemcpyAsync(out, addend, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  if (kernel) return launch_ckks_const_mac_sum(c, ct.data(), ct_nl.data(), w, (int)ct.size(), cst, addend, out, size, nl, count);
  bool raised = false;
  for (int l : ct_nl) raised |= l > nl;
  if (ensure_aux(c, 6, (pw + (raised ? words : 0)) * 8)) return 1;
  if ((addend || ct.size() > 1) && ensure_aux(c, 2, bytes)) return 1;
  u64 *plain = (u64 *)c->aux[6], *lowered = plain + pw;
  const u64 *carry = addend;
  for (size_t k = 0; k < ct.size(); k++) {
    const u64 *src = ct[k];
    if (ct_nl[k] > nl) {
      if (launch_drop_to(c, src, lowered, ct_nl[k], nl, count * size)) return 1;
      src = lowered;
    }
    if (launch_const_plain_fill(c, w + k * nl, plain, nl)) return 1;
    u64 *dst = carry ? (u64 *)c->aux[2] : out;
    if (ckks_multiply_plain(c, src, plain, 0, dst, size, nl, count)) return 1;
    if (carry && launch_addsub(c, carry, dst, out, nl, count * size, 0)) return 1;
    carry = out;
  }
  if (cst) {
    if (!carry) {
      ABC_HIP_CHECK(hipMemsetAsync(out, 0, bytes, c->stream));
      carry = out;
    }
    if (launch_const_plain_fill(c, cst, plain, nl)) return 1;
    if (ckks_add_plain(c, carry, plain, 0, out, size, nl, count, 0)) return 1;
  }
  return 0;
}

// out [count][size][nl-1][N] = rescale(const_mac_sum(...)) (CKKS, nl >= 2); out overlaps no operand (the caller has checked).  Fused
// (route_const_sum_rescale: up to four terms, all at nl, where the measurement has it faster): the K-term forms of the two
// LDS-resident rescale kernels take addend, constant and terms, and the sum never reaches memory.  Separate: the whole sum into arena
// 1, then launch_rescale; arenas 2 and 6 are const_mac_sum's on its composed route.
static int const_sum_rescale(abc_hip_ctx *c, const std::vector<const u64 *> &ct, const std::vector<int> &ct_nl, const u64 *w, const u64 *cst,
                             const u64 *addend, u64 *out, int size, int nl, size_t count) {
  if (!count) return 0;
  const size_t N = (size_t)c->n, in_bytes = count * size * (size_t)nl * N * 8;
  if (ct.empty() && !cst && !addend) {  // rescale(0) = 0
    ABC_HIP_CHECK(hipMemsetAsync(out, 0, count * size * (size_t)(nl - 1) * N * 8, c->stream));
    return 0;
  }
  if (ct.empty() && !cst) return launch_rescale(c, addend, out, size, nl, count);
  bool raised = false;
  for (int l : ct_nl) raised |= l > nl;
  const ConstSumRescaleRoute r = route_const_sum_rescale(c->facts, nl, count * size, (int)ct.size(), raised);
  if (r.fused) return launch_const_sum_rescale(c, r.rescale, ct.data(), w, (int)ct.size(), cst, addend, out, size, nl, count);
  if (ensure_aux(c, 1, in_bytes)) return 1;
  u64 *sum = (u64 *)c->aux[1];
  if (const_mac_sum(c, route_const_mac_sum(c->facts, nl), ct, ct_nl, w, cst, addend, sum, size, nl, count)) return 1;
  return launch_rescale(c, sum, out, size, nl, count);
}

// out = sum_j rotate( sum_i D[j * n_baby + i] (.) rotate(in, baby[i]), giant[j] ), in the order given (abc_hip.h).  The batch goes
// in groups of ciphertexts (matvec_bsgs_group).  Per group: the baby rotations land in arena 3, one slab per non-zero step (step 0
// is the input itself); per giant step the inner sum over the slabs lands in arena 4 and one rotate_tail adds its rotation to the
// group's slice of `out` -- the first giant step writes the slice, a giant step of 0 has no rotation: its inner sum is formed
// onto the slice directly.  Arenas 0 .. 2 belong to the rotations (and to the per-term inner sum between them).
// BFV (abc_hip_bfv_diag_matvec_bsgs; diags in NTT form, bfv_plain_to_ntt): the slabs are transformed to NTT form once -- the rotated
// ones in place, in one launch where the group fills its slabs; step 0 gets a slab of its own behind them, a transformed copy,
// because `in` stays untouched -- and every inner sum is bfv_multiply_plain_sum on NTT-form terms: no forward transform at all
// (arena 2: its partial sum, or its sum under an addend).
static int diag_matvec_bsgs(abc_hip_ctx *c, const u64 *in, const u64 *diags, size_t diag_stride, const std::vector<int> &baby,
                            const std::vector<int> &giant, u64 *out, int nl, size_t count) {
  const size_t pw = (size_t)nl * c->n, bytes = count * 2 * pw * 8;
  if (check_steps(c, baby) || check_steps(c, giant)) return 1;
  if (!count) return 0;
  if (ranges_overlap(in, bytes, out, bytes)) { set_error("diag_matvec_bsgs: d_out must not overlap d_in"); return 1; }
  if (baby.empty() || giant.empty()) {
    ABC_HIP_CHECK(hipMemsetAsync(out, 0, bytes, c->stream));
    return 0;
  }
  const bool bfv = c->scheme == ABC_HIP_SCHEME_BFV;
  const MatvecBsgsRoute r = route_matvec_bsgs(c->facts, nl);
  const LimbMap qmap = bfv ? key_limb_map(c, nl) : LimbMap{};  // the BFV transforms alone read it
  const size_t nb = baby.size();
  size_t rotated = 0;
  for (int s : baby) rotated += s != 0;
  const size_t slabs = bfv ? nb : rotated;
  const size_t group = matvec_bsgs_group(c->facts, nl, count, (int)slabs);
  if (slabs && ensure_aux(c, 3, slabs * group * 2 * pw * 8)) return 1;
  bool inner_arena = false;
  for (int g : giant) inner_arena |= g != 0;
  if (inner_arena && ensure_aux(c, 4, group * 2 * pw * 8)) return 1;
  std::vector<const u64 *> x(nb), d(nb);
  auto inner_sum = [&](const u64 *addend, u64 *dst, size_t cc) {
    return bfv ? bfv_multiply_plain_sum(c, x.data(), true, d.data(), 0, (int)nb, addend, dst, 2, cc) : plain_mac_sum(c, r.macsum, x, d, 0, addend, dst, 2, nl, cc);
  };
  for (size_t off = 0; off < count; off += group) {
    const size_t cc = count - off < group ? count - off : group;
    const u64 *gin = in + off * 2 * pw;
    u64 *gout = out + off * 2 * pw;
    size_t slab = 0, copies = rotated;
    for (size_t i = 0; i < nb; i++) {
      if (!baby[i]) {
        x[i] = gin;
        if (bfv) {
          u64 *dst = (u64 *)c->aux[3] + copies++ * group * 2 * pw;
          if (launch_ntt_fwd_from(c, gin, dst, qmap, nl, cc * 2 * nl)) return 1;
          x[i] = dst;
        }
        continue;
      }
      u64 *dst = (u64 *)c->aux[3] + slab++ * group * 2 * pw;
      if (rotate_tail(c, gin, {}, dst, nl, baby[i], cc)) return 1;
      x[i] = dst;
    }
    if (bfv && rotated) {
      if (cc == group) {
        if (launch_ntt_fwd(c, (u64 *)c->aux[3], qmap, nl, rotated * cc * 2 * nl)) return 1;
      } else {  // a ragged last group leaves gaps between its slabs
        for (size_t s = 0; s < rotated; s++)
          if (launch_ntt_fwd(c, (u64 *)c->aux[3] + s * group * 2 * pw, qmap, nl, cc * 2 * nl)) return 1;
      }
    }
    for (size_t j = 0; j < giant.size(); j++) {
      for (size_t i = 0; i < nb; i++) d[i] = diags + (j * nb + i) * diag_stride;
      if (!giant[j]) {
        if (inner_sum(j ? gout : nullptr, gout, cc)) return 1;
        continue;
      }
      u64 *inner = (u64 *)c->aux[4];
      if (inner_sum(nullptr, inner, cc)) return 1;
      if (rotate_tail(c, inner, {j ? gout : nullptr}, gout, nl, giant[j], cc)) return 1;
    }
  }
  return 0;
}

// out [count][2][nl-1][N] = sum_j rotate( rescale( sum_i D[j * n_baby + i] (.) rotate(in, baby[i]) ), giant[j] ) (CKKS, nl >= 2):
// diag_matvec_bsgs with every inner sum rescaled before its giant rotation.  Groups and the baby arena (3) as there; per giant step
// one plain_sum_rescale into arena 4 (nl - 1 limbs) and one rotate_tail at nl - 1 onto the group's slice of `out`; a giant step of 0
// writes the slice where it is the first, else its rescaled inner sum goes to arena 4 and the add kernel follows.
static int diag_matvec_bsgs_rescale(abc_hip_ctx *c, const u64 *in, const u64 *diags, size_t diag_stride, const std::vector<int> &baby,
                                    const std::vector<int> &giant, u64 *out, int nl, size_t count) {
  const size_t pw = (size_t)nl * c->n, ow = (size_t)(nl - 1) * c->n;
  if (check_steps(c, baby) || check_steps(c, giant)) return 1;
  if (!count) return 0;
  if (ranges_overlap(in, count * 2 * pw * 8, out, count * 2 * ow * 8)) { set_error("diag_matvec_bsgs_rescale: d_out must not overlap d_in"); return 1; }
  if (baby.empty() || giant.empty()) {
    ABC_HIP_CHECK(hipMemsetAsync(out, 0, count * 2 * ow * 8, c->stream));
    return 0;
  }
  const size_t nb = baby.size();
  size_t slabs = 0;
  for (int s : baby) slabs += s != 0;
  const size_t group = matvec_bsgs_group(c->facts, nl, count, (int)slabs);
  if (slabs && ensure_aux(c, 3, slabs * group * 2 * pw * 8)) return 1;
  bool inner_arena = false;
  for (size_t j = 0; j < giant.size(); j++) inner_arena |= giant[j] != 0 || j != 0;
  if (inner_arena && ensure_aux(c, 4, group * 2 * ow * 8)) return 1;
  std::vector<const u64 *> x(nb), d(nb);
  for (size_t off = 0; off < count; off += group) {
    const size_t cc = count - off < group ? count - off : group;
    const u64 *gin = in + off * 2 * pw;
    u64 *gout = out + off * 2 * ow;
    size_t slab = 0;
    for (size_t i = 0; i < nb; i++) {
      if (!baby[i]) {
        x[i] = gin;
        continue;
      }
      u64 *dst = (u64 *)c->aux[3] + slab++ * group * 2 * pw;
      if (rotate_tail(c, gin, {}, dst, nl, baby[i], cc)) return 1;
      x[i] = dst;
    }
    for (size_t j = 0; j < giant.size(); j++) {
      for (size_t i = 0; i < nb; i++) d[i] = diags + (j * nb + i) * diag_stride;
      if (!giant[j] && !j) {
        if (plain_sum_rescale(c, x, d, 0, nullptr, gout, 2, nl, cc)) return 1;
        continue;
      }
      u64 *inner = (u64 *)c->aux[4];
      if (plain_sum_rescale(c, x, d, 0, nullptr, inner, 2, nl, cc)) return 1;
      if (!giant[j] ? launch_addsub(c, gout, inner, gout, nl - 1, cc * 2, 0) : rotate_tail(c, inner, {j ? gout : nullptr}, gout, nl - 1, giant[j], cc)) return 1;
    }
  }
  return 0;
}

}  // namespace abc

using namespace abc;

// roctx range around every C-ABI operation (rocprofv3 --marker-trace then shows the op boundaries above the kernel rows; the
// reference's only instrumentation is four wall-clock phase timers, examples/main.cpp:41).  The marker library is bound with
// dlopen on first use -- libabc_hip.so carries no link-time dependency on a profiler -- and ABC_HIP_NO_ROCTX=1 skips it.
namespace abc {
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (env_on("ABC_HIP_NO_ROCTX")) return;
    for (const char *lib : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      if (void *h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL)) {
        push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
  }
};
static const Roctx &roctx() {
  static const Roctx r;
  return r;
}
struct OpRange {
  bool on;
  explicit OpRange(const char *name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~OpRange() {
    if (on) roctx().pop();
  }
};
// the one place every C-ABI entry passes: the outermost one of a call poisons the scratch arenas (ABC_HIP_POISON=1); a composite
// call that re-enters the C ABI is deeper and keeps what it has built there
struct OpDepth {
  abc_hip_ctx *c;
  explicit OpDepth(abc_hip_ctx *c_) : c(c_ && c_->poison ? c_ : nullptr) {
    if (c && c->op_depth++ == 0 && hipSetDevice(c->device) == hipSuccess) poison_arenas(c);
  }
  ~OpDepth() {
    if (c) c->op_depth--;
  }
};
}  // namespace abc

#define CTX_GUARD(c)                                   \
  abc::OpRange abc_op_range_(__func__);                \
  abc::OpDepth abc_op_depth_(c);                       \
  do {                                                 \
    if (!(c)) { set_error("null context"); return 1; } \
    if (hipSetDevice((c)->device) != hipSuccess) { set_error("hipSetDevice failed"); return 1; } \
  } while (0)

// no exception crosses the C boundary: what() becomes the error text of a failed call
template <class F>
static int guarded(F &&body) {
  try {
    return body();
  } catch (const std::exception &e) {
    set_error(e.what());
    return 1;
  }
}

extern "C" {

const char *abc_hip_last_error(void) { return g_err.c_str(); }

int abc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int abc_hip_default_bfv_primes(size_t n, uint64_t *out) {
  // the 128-bit-security default chains of SEAL 3.6 (CoeffModulus::BFVDefault)
  static const uint64_t p1024[] = {0x7e00001ull};
  static const uint64_t p2048[] = {0x3fffffff000001ull};
  static const uint64_t p4096[] = {0xffffee001ull, 0xffffc4001ull, 0x1ffffe0001ull};
  static const uint64_t p8192[] = {0x7fffffd8001ull, 0x7fffffc8001ull, 0xfffffffc001ull, 0xffffff6c001ull, 0xfffffebc001ull};
  static const uint64_t p16384[] = {0xfffffffd8001ull,  0xfffffffa0001ull,  0xfffffff00001ull,  0x1fffffff68001ull, 0x1fffffff50001ull,
                                    0x1ffffffee8001ull, 0x1ffffffea0001ull, 0x1ffffffe88001ull, 0x1ffffffe48001ull};
  static const uint64_t p32768[] = {0x7fffffffe90001ull, 0x7fffffffbf0001ull, 0x7fffffffbd0001ull, 0x7fffffffba0001ull,
                                    0x7fffffffaa0001ull, 0x7fffffffa50001ull, 0x7fffffff9f0001ull, 0x7fffffff7e0001ull,
                                    0x7fffffff770001ull, 0x7fffffff380001ull, 0x7fffffff330001ull, 0x7fffffff2d0001ull,
                                    0x7fffffff170001ull, 0x7fffffff150001ull, 0x7ffffffef00001ull, 0xfffffffff70001ull};
  const uint64_t *src = nullptr;
  int cnt = 0;
  switch (n) {
    case 1024: src = p1024; cnt = 1; break;
    case 2048: src = p2048; cnt = 1; break;
    case 4096: src = p4096; cnt = 3; break;
    case 8192: src = p8192; cnt = 5; break;
    case 16384: src = p16384; cnt = 9; break;
    case 32768: src = p32768; cnt = 16; break;
    default: set_error("no default BFV coefficient modulus for this ring degree"); return -1;
  }
  for (int i = 0; i < cnt; i++) out[i] = src[i];
  return cnt;
}

uint64_t abc_hip_plain_modulus_batching(size_t n, int bits) {
  try {
    return host::ntt_primes(n, bits, 1)[0];
  } catch (const std::exception &e) {
    set_error(e.what());
    return 0;
  }
}

int abc_hip_create_primes(size_t n, const int *bit_sizes, int count, uint64_t *out) {
  return guarded([&] {
    std::map<int, std::vector<uint64_t>> table;
    for (int i = 0; i < count; i++) table[bit_sizes[i]];
    for (auto &kv : table) {
      size_t need = 0;
      for (int i = 0; i < count; i++) need += (bit_sizes[i] == kv.first);
      kv.second = host::ntt_primes(n, kv.first, need);
    }
    for (int i = 0; i < count; i++) {  // hand out from the back (smallest first), as CoeffModulus::Create does
      auto &v = table[bit_sizes[i]];
      out[i] = v.back();
      v.pop_back();
    }
    return 0;
  });
}

int abc_hip_ctx_create(int scheme, int logn, const uint64_t *primes, int nprimes, uint64_t plain_modulus, int device,
                       abc_hip_ctx **out) {
  if (!out) { set_error("null output pointer"); return 1; }
  *out = nullptr;
  if (scheme != ABC_HIP_SCHEME_BFV && scheme != ABC_HIP_SCHEME_CKKS) { set_error("unknown scheme"); return 1; }
  if (logn < 10 || logn > 16) { set_error("logn must be in 10..16"); return 1; }
  if (nprimes < 2 || nprimes > kMaxLimbs) { set_error("need 2..16 primes (data limbs + special prime)"); return 1; }
  const uint64_t two_n = 2ull << logn;
  for (int i = 0; i < nprimes; i++) {
    if (primes[i] >> 60 || !host::is_prime(primes[i]) || primes[i] % two_n != 1) {
      set_error("coefficient modulus primes must be < 2^60, prime and = 1 mod 2N");
      return 1;
    }
    for (int j = 0; j < i; j++)
      if (primes[j] == primes[i]) { set_error("coefficient modulus primes must be distinct"); return 1; }
  }
  if (scheme == ABC_HIP_SCHEME_BFV) {
    if (!host::is_prime(plain_modulus) || plain_modulus % two_n != 1 || plain_modulus >> 32) {
      set_error("plain modulus must be a prime = 1 mod 2N (batching) below 2^32");
      return 1;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available"); return 1; }
  if (device < 0 || device >= ndev) { set_error("device index out of range"); return 1; }
  if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice failed"); return 1; }
  abc_hip_ctx *c = new abc_hip_ctx();
  c->scheme = scheme; c->logn = logn; c->n = 1 << logn; c->K = nprimes; c->L = nprimes - 1; c->device = device;
  c->primes.assign(primes, primes + nprimes);
  c->t = (scheme == ABC_HIP_SCHEME_BFV) ? plain_modulus : 0;
  int rc = 1;
  try {
    rc = build_context(c);
  } catch (const std::exception &e) {
    set_error(e.what());
  }
  if (!rc && hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("hipStreamCreate failed");
    rc = 1;
  }
  if (!rc) c->stream = c->own_stream;  // operations run on a private stream unless abc_hip_set_stream overrides it
  if (!rc && (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
              hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming) != hipSuccess)) {
    set_error("hipEventCreate failed");
    rc = 1;
  }
  for (int i = 0; !rc && i < abc_hip_ctx::kMaxLanes; i++) {
    if (hipStreamCreateWithFlags(&c->lane[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->lane_join[i], hipEventDisableTiming) != hipSuccess) {
      set_error("lane stream / event creation failed");
      rc = 1;
    }
  }
  if (!rc && !env_on("ABC_HIP_SYNC_ALLOC")) {
    c->cache_alloc = true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) c->buffers.cache_cap = total_b / 4;  // at most a quarter of the device
  }
  if (!rc) c->poison = env_on("ABC_HIP_POISON");
  if (rc) { abc_hip_ctx_destroy(c); return 1; }
  *out = c;
  return 0;
}

void abc_hip_ctx_destroy(abc_hip_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(c->d_mods); (void)hipFree(c->d_tw); (void)hipFree(c->d_ftw); (void)hipFree(c->d_cst); (void)hipFree(c->d_cstf);
  (void)hipFree(c->d_slot_map);
  (void)hipFree(c->d_ckks_codec);
  (void)hipFree(c->d_crt);
  // workspace, arenas, keys, key mirrors, what is held back for a graph never destroyed, and every block abc_hip_malloc
  // handed out and that was not returned to the driver: cached ones and ones the caller still holds (a caller that frees after
  // destroying the context would otherwise leak them)
  free_buffers(c);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->lane_fork) (void)hipEventDestroy(c->lane_fork);
  for (int i = 0; i < abc_hip_ctx::kMaxLanes; i++) {
    if (c->lane_join[i]) (void)hipEventDestroy(c->lane_join[i]);
    if (c->lane[i]) (void)hipStreamDestroy(c->lane[i]);
  }
  delete c;
}

int abc_hip_ctx_info(const abc_hip_ctx *c, int what) {
  if (!c) return -1;
  switch (what) {
    case 0: return c->scheme;
    case 1: return c->logn;
    case 2: return c->K;
    case 3: return c->L;
    case 4: return c->device;
    case 5: return c->nBsk;
    case 6: return held_buffers(c);
    default: return -1;
  }
}

int abc_hip_set_stream(abc_hip_ctx *c, void *stream) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_set_stream");
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->stream = stream ? (hipStream_t)stream : c->own_stream;  // NULL selects the context's private stream again
  return 0;
}
int abc_hip_sync(abc_hip_ctx *c) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_sync");
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

// allocator and graph lifetime: abc_buffers.hip
int abc_hip_malloc(abc_hip_ctx *c, void **d_ptr, size_t bytes) { CTX_GUARD(c); return buffer_malloc(c, d_ptr, bytes); }
int abc_hip_free(abc_hip_ctx *c, void *d_ptr) { CTX_GUARD(c); return buffer_free(c, d_ptr); }
int abc_hip_trim(abc_hip_ctx *c) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_trim");
  return trim_cache(c);
}
size_t abc_hip_cached_bytes(abc_hip_ctx *c) { return c ? cached_bytes(c) : 0; }
int abc_hip_ctx_reload_env(abc_hip_ctx *c) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_ctx_reload_env");
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  read_switches(c);
  return 0;
}
int abc_hip_memcpy_h2d(abc_hip_ctx *c, void *d, const void *h, size_t bytes) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_memcpy_h2d");
  ABC_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
int abc_hip_memcpy_d2h(abc_hip_ctx *c, void *h, const void *d, size_t bytes) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_memcpy_d2h");
  ABC_HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
int abc_hip_memcpy_d2d(abc_hip_ctx *c, void *dst, const void *src, size_t bytes) {
  CTX_GUARD(c);
  ABC_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// ---- keys ----
int abc_hip_keygen(abc_hip_ctx *c, uint64_t seed) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_keygen");
  return guarded([&] { return keygen(c, seed); });
}
int abc_hip_keygen_secure(abc_hip_ctx *c) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_keygen_secure");
  return guarded([&] { return keygen_secure(c); });
}
int abc_hip_keygen_keyed(abc_hip_ctx *c, const uint8_t key_sec[32], const uint8_t key_pub[32]) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_keygen_keyed");
  return guarded([&] { return keygen_keyed(c, key_sec, key_pub); });
}
// A key is rewritten in place, and so are its mirrors: a recorded circuit keeps the addresses it baked in and reads the new key on
// its next replay.  Work already enqueued (a replay among it) finishes on the old words first: the stream is non-blocking, so the
// synchronous copy below would not wait for it.
static int load_key(abc_hip_ctx *c, uint64_t **slot, const uint64_t *h, size_t words) {
  NOT_CAPTURABLE(c, "key upload");
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  const bool fresh = !*slot;
  if (fresh) ABC_HIP_CHECK(alloc_context_buffer(c, (void **)slot, words * 8, false));
  ABC_HIP_CHECK(hipMemcpy(*slot, h, words * 8, hipMemcpyHostToDevice));
  if (!fresh && refresh_key_mirrors(c, *slot)) return 1;
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
int abc_hip_load_secret_key(abc_hip_ctx *c, const uint64_t *h) { CTX_GUARD(c); return load_key(c, &c->d_sk, h, (size_t)c->K * c->n); }
int abc_hip_load_public_key(abc_hip_ctx *c, const uint64_t *h) { CTX_GUARD(c); return load_key(c, &c->d_pk, h, (size_t)2 * c->K * c->n); }
int abc_hip_load_relin_key(abc_hip_ctx *c, const uint64_t *h) { CTX_GUARD(c); return load_key(c, &c->d_relin, h, c->key_words()); }
int abc_hip_load_galois_key(abc_hip_ctx *c, uint32_t elt, const uint64_t *h) {
  CTX_GUARD(c);
  if (!(elt & 1) || elt >= 2u * (uint32_t)c->n) { set_error("Galois element must be odd and below 2N"); return 1; }
  uint64_t *slot = c->d_galois.count(elt) ? c->d_galois[elt] : nullptr;
  const bool fresh = (slot == nullptr);
  if (load_key(c, &slot, h, c->key_words())) return 1;
  c->d_galois[elt] = slot;
  if (fresh) c->galois_order.push_back(elt);
  return 0;
}
static int get_key(abc_hip_ctx *c, const uint64_t *d, uint64_t *h, size_t words, const char *what) {
  NOT_CAPTURABLE(c, "key download");
  if (!d) { set_error(std::string("key not present: ") + what); return 1; }
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  ABC_HIP_CHECK(hipMemcpy(h, d, words * 8, hipMemcpyDeviceToHost));
  return 0;
}
int abc_hip_get_secret_key(abc_hip_ctx *c, uint64_t *h) { CTX_GUARD(c); return get_key(c, c->d_sk, h, (size_t)c->K * c->n, "secret"); }
int abc_hip_get_public_key(abc_hip_ctx *c, uint64_t *h) { CTX_GUARD(c); return get_key(c, c->d_pk, h, (size_t)2 * c->K * c->n, "public"); }
int abc_hip_get_relin_key(abc_hip_ctx *c, uint64_t *h) { CTX_GUARD(c); return get_key(c, c->d_relin, h, c->key_words(), "relin"); }
int abc_hip_get_galois_key(abc_hip_ctx *c, uint32_t elt, uint64_t *h) {
  CTX_GUARD(c);
  auto it = c->d_galois.find(elt);
  return get_key(c, it == c->d_galois.end() ? nullptr : it->second, h, c->key_words(), "galois");
}
int abc_hip_num_galois_keys(abc_hip_ctx *c) { return c ? (int)c->galois_order.size() : 0; }
uint32_t abc_hip_galois_elt_at(abc_hip_ctx *c, int i) {
  if (!c || i < 0 || i >= (int)c->galois_order.size()) return 0;
  return c->galois_order[i];
}
uint32_t abc_hip_galois_elt_from_step(abc_hip_ctx *c, int step) { return c ? elt_from_step(c, step) : 0; }

// ---- encode / encrypt / decrypt ----
int abc_hip_batch_encode(abc_hip_ctx *c, const int64_t *v, uint64_t *p, size_t count) { CTX_GUARD(c); return batch_encode(c, v, p, count); }
int abc_hip_batch_decode(abc_hip_ctx *c, const uint64_t *p, int64_t *v, size_t count) { CTX_GUARD(c); return batch_decode(c, p, v, count); }
int abc_hip_ckks_encode(abc_hip_ctx *c, const double *re, const double *im, size_t values_per_row, double scale, int nl, uint64_t *p,
                        size_t count) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_ckks_encode");
  return ckks_encode(c, re, im, values_per_row, scale, nl, p, count);
}
int abc_hip_ckks_decode(abc_hip_ctx *c, const uint64_t *p, int nl, double scale, double *re, double *im, size_t count) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_ckks_decode");
  return ckks_decode(c, p, nl, scale, re, im, count);
}
int abc_hip_encrypt(abc_hip_ctx *c, const uint64_t *p, uint64_t seed, uint64_t *ct, size_t count) { CTX_GUARD(c); NOT_CAPTURABLE(c, "abc_hip_encrypt"); return guarded([&] { return encrypt(c, p, seed, ct, count); }); }
int abc_hip_encrypt_secure(abc_hip_ctx *c, const uint64_t *p, uint64_t *ct, size_t count) { CTX_GUARD(c); NOT_CAPTURABLE(c, "abc_hip_encrypt_secure"); return guarded([&] { return encrypt_secure(c, p, ct, count); }); }
int abc_hip_encrypt_keyed(abc_hip_ctx *c, const uint64_t *p, const uint8_t key[32], uint64_t nonce, uint64_t *ct, size_t count) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_encrypt_keyed");
  return guarded([&] { return encrypt_keyed(c, p, key, nonce, ct, count); });
}
int abc_hip_keyed_small(abc_hip_ctx *c, const uint8_t key[32], uint64_t nonce, int8_t *d_small, size_t count) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_keyed_small");
  return guarded([&] { return keyed_small(c, key, nonce, d_small, count); });
}
int abc_hip_keyed_uniform(abc_hip_ctx *c, const uint8_t key[32], uint64_t stream, int nkeys, uint64_t *d_a) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_keyed_uniform");
  return guarded([&] { return keyed_uniform(c, key, stream, nkeys, d_a); });
}
int abc_hip_keyed_small_host(const uint8_t key[32], uint64_t nonce, size_t n, size_t count, int8_t *h_small) {
  if (!key || (!h_small && count)) { set_error("keyed_small_host: null pointer"); return 1; }
  if (!n || n % 8) { set_error("keyed_small_host: n must be a positive multiple of 8"); return 1; }
  keyed::encrypt_small_host(key, nonce, n, count, h_small);
  return 0;
}
int abc_hip_decrypt(abc_hip_ctx *c, const uint64_t *ct, int size, int nl, uint64_t *p, size_t count) {
  CTX_GUARD(c);
  if (nl < 1 || nl > c->L) { set_error("decrypt: bad limb count"); return 1; }
  return decrypt(c, ct, size, nl, p, count);
}
int abc_hip_noise_budget(abc_hip_ctx *c, const uint64_t *ct, int size, int nl, int *h_budget, size_t count) {
  CTX_GUARD(c);
  NOT_CAPTURABLE(c, "abc_hip_noise_budget");
  return noise_budget(c, ct, size, nl, h_budget, count);
}

// ---- evaluator ----
static int check_level(abc_hip_ctx *c, int nl) {
  if (nl < 1 || nl > c->L) { set_error("limb count out of range for this context"); return 1; }
  if (c->scheme == ABC_HIP_SCHEME_BFV && nl != c->L) { set_error("BFV ciphertexts live at the top level (nl = L)"); return 1; }
  return 0;
}
// one plaintext for the batch (0) or one per ciphertext; any other stride would read past a row or overlap two (abc_hip.h)
static int check_plain_stride(abc_hip_ctx *c, const char *op, size_t plain_stride, int nl) {
  if (!plain_stride) return 0;
  const bool ckks = c->scheme == ABC_HIP_SCHEME_CKKS;
  if (ckks ? plain_stride >= (size_t)nl * c->n : plain_stride == (size_t)c->n) return 0;
  set_error(std::string(op) + (ckks ? ": plain_stride must be 0 or at least nl * N" : ": plain_stride must be 0 or N"));
  return 1;
}
// what the plaintext calls check before anything else: a CKKS context, the stride, and that `plain` (rows of nl * N words, `rows`
// of them `stride` apart) stays clear of the `out_words` words at `out`
static int check_mac_plain(abc_hip_ctx *c, const char *op, const u64 *plain, size_t stride, size_t rows, const u64 *out, size_t out_words,
                           int nl) {
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error(std::string(op) + ": CKKS only (a BFV plaintext product needs transforms and is no fold of the key switch)"); return 1; }
  if (check_plain_stride(c, op, stride, nl)) return 1;
  const size_t plain_words = rows ? (rows - 1) * stride + (size_t)nl * c->n : 0;
  if (plain_words && out_words && ranges_overlap(plain, plain_words * 8, out, out_words * 8)) { set_error(std::string(op) + ": the plaintext must not overlap d_out"); return 1; }
  return 0;
}

int abc_hip_route(abc_hip_ctx *c, int op, int nl, size_t count, int in_place, char *buf, size_t cap) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;  // nl as the operation itself takes it (BFV: L, also for multiply)
  if (op == kRouteRescale && (nl < 2 || c->scheme != ABC_HIP_SCHEME_CKKS)) { set_error("route: rescale needs CKKS and nl >= 2"); return 1; }
  if (op == kRouteMulPlainRescale && (nl < 2 || c->scheme != ABC_HIP_SCHEME_CKKS)) { set_error("route: multiply_plain_rescale needs CKKS and nl >= 2"); return 1; }
  if (op == kRouteDiagMatvecBsgs && c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("route: diag_matvec_bsgs needs CKKS"); return 1; }
  if ((op == kRoutePlainSumRescale || op == kRouteDiagMatvecBsgsRescale) && (nl < 2 || c->scheme != ABC_HIP_SCHEME_CKKS)) { set_error("route: multiply_plain_sum_rescale and diag_matvec_bsgs_rescale need CKKS and nl >= 2"); return 1; }
  if ((op == kRouteConstSumRescale || op == kRoutePolyEval) && (nl < 2 || c->scheme != ABC_HIP_SCHEME_CKKS)) { set_error("route: multiply_const_sum_rescale and ckks_poly_eval need CKKS and nl >= 2"); return 1; }
  if ((op == kRouteBfvPlainSum || op == kRouteBfvMatvecBsgs) && c->scheme != ABC_HIP_SCHEME_BFV) { set_error("route: bfv_multiply_plain_sum and bfv_diag_matvec_bsgs need BFV"); return 1; }
  const int n = !buf                        ? -1
                : op == kRouteDiagMatvecBsgs ? format_matvec_bsgs(buf, cap, c->facts, nl, count)
                : op == kRoutePlainSumRescale ? format_plain_sum_rescale(buf, cap, c->facts, nl, count)
                : op == kRouteDiagMatvecBsgsRescale ? format_matvec_bsgs_rescale(buf, cap, c->facts, nl, count)
                : op == kRouteConstSumRescale ? format_const_sum_rescale(buf, cap, c->facts, nl, count)
                : op == kRoutePolyEval       ? format_poly_eval(buf, cap, c->facts, nl, count)
                : op == kRouteBfvPlainSum    ? format_bfv_plain_sum(buf, cap, c->facts, count)
                : op == kRouteBfvMatvecBsgs  ? format_bfv_matvec_bsgs(buf, cap, c->facts, count)
                                             : format_op(buf, cap, c->facts, op, nl, count, in_place != 0);
  if (n == -2) { set_error("route: unknown operation"); return 1; }
  if (n < 0) { set_error("route: buffer too small"); return 1; }
  return 0;
}
int abc_hip_add(abc_hip_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return launch_addsub(c, a, b, out, nl, count * size, 0);
}
int abc_hip_sub(abc_hip_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return launch_addsub(c, a, b, out, nl, count * size, 1);
}
int abc_hip_negate(abc_hip_ctx *c, const uint64_t *a, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return launch_addsub(c, a, nullptr, out, nl, count * size, 2);
}
int abc_hip_multiply(abc_hip_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out3, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (c->scheme == ABC_HIP_SCHEME_CKKS) return launch_ckks_tensor(c, a, b, out3, nl, count);
  return bfv_multiply(c, route_bfv_multiply(c->facts), a, b, out3, count);
}
int abc_hip_relinearize(abc_hip_ctx *c, const uint64_t *ct3, uint64_t *out2, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return relinearize(c, ct3, out2, nl, count);
}
// multiply + relinearise along the route of the level; the caller has checked the level and the key (abc_hip_mul_relin, and every
// product of ckks_poly_eval)
static int mul_relin(abc_hip_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int nl, size_t count) {
  const MulRoute r = route_mul_relin(c->facts, nl);
  if (r.seq == Seq::bmul) return bmul_split(c, a, b, out, count, true);
  if (r.seq != Seq::generic) return launch_mul_relin(c, r.seq, a, b, out, nl, count);
  // generic path: size-3 product in arena 1, then key switch
  const size_t bytes = count * 3 * nl * (size_t)c->n * 8;
  if (ensure_aux(c, 1, bytes ? bytes : 8)) return 1;
  u64 *t3 = (u64 *)c->aux[1];
  int rc = (c->scheme == ABC_HIP_SCHEME_CKKS) ? launch_ckks_tensor(c, a, b, t3, nl, count) : bfv_multiply(c, r.mul, a, b, t3, count);
  if (!rc) rc = launch_keyswitch(c, r.ks, ks_of_ciphertexts(c, t3, 3, c->d_relin, out, nl, count));  // as in relinearize
  return rc;
}
int abc_hip_mul_relin(abc_hip_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (!c->d_relin) { set_error("mul_relin: no relinearisation key"); return 1; }
  return mul_relin(c, a, b, out, nl, count);
}
// what both sum-of-products calls check before anything is written or enqueued; exact_ok: a term may BE d_out (mul_sum_relin)
static int check_mul_sum(abc_hip_ctx *c, const char *op, const uint64_t *const *h_a, const uint64_t *const *h_b, int n_terms, const uint64_t *out,
                         int out_size, bool exact_ok, int nl, size_t count) {
  if (check_level(c, nl)) return 1;
  if (n_terms < 0 || (n_terms && (!h_a || !h_b))) { set_error(std::string(op) + ": bad term list"); return 1; }
  const size_t pw = (size_t)nl * c->n;
  for (int k = 0; k < n_terms; k++) {
    if (!h_a[k] || !h_b[k]) { set_error(std::string(op) + ": null term pointer"); return 1; }
    for (const uint64_t *t : {h_a[k], h_b[k]}) {
      if (exact_ok && t == out) continue;
      if (count && ranges_overlap(t, count * 2 * pw * 8, out, count * out_size * pw * 8)) {
        set_error(std::string(op) + (exact_ok ? ": d_out may be a term, but must not overlap one otherwise" : ": d_out3 must not overlap a term"));
        return 1;
      }
    }
  }
  if (!out && count) { set_error(std::string(op) + ": null output"); return 1; }
  return 0;
}
int abc_hip_multiply_sum(abc_hip_ctx *c, const uint64_t *const *h_a, const uint64_t *const *h_b, int n_terms, uint64_t *out3, int nl,
                         size_t count) {
  CTX_GUARD(c);
  if (check_mul_sum(c, "multiply_sum", h_a, h_b, n_terms, out3, 3, false, nl, count)) return 1;
  return guarded([&] {
    return mul_sum(c, std::vector<const u64 *>(h_a, h_a + n_terms), std::vector<const u64 *>(h_b, h_b + n_terms), out3, false, nl, count);
  });
}
int abc_hip_mul_sum_relin(abc_hip_ctx *c, const uint64_t *const *h_a, const uint64_t *const *h_b, int n_terms, uint64_t *out, int nl,
                          size_t count) {
  CTX_GUARD(c);
  if (check_mul_sum(c, "mul_sum_relin", h_a, h_b, n_terms, out, 2, true, nl, count)) return 1;
  if (!c->d_relin) { set_error("mul_sum_relin: no relinearisation key"); return 1; }
  return guarded([&] {
    return mul_sum(c, std::vector<const u64 *>(h_a, h_a + n_terms), std::vector<const u64 *>(h_b, h_b + n_terms), out, true, nl, count);
  });
}
int abc_hip_rotate(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int nl, int steps, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return guarded([&] { return rotate_tail(c, in, {}, out, nl, steps, count); });
}
int abc_hip_apply_galois(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int nl, uint32_t elt, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (in == out) { set_error("apply_galois: in-place not supported, use abc_hip_rotate"); return 1; }
  return guarded([&] { return apply_galois_tail(c, in, {}, out, nl, elt, count, 1); });
}
int abc_hip_rotate_add(abc_hip_ctx *c, const uint64_t *in, const uint64_t *addend, uint64_t *out, int nl, int steps, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return guarded([&] { return rotate_tail(c, in, {addend}, out, nl, steps, count); });
}
int abc_hip_apply_galois_add(abc_hip_ctx *c, const uint64_t *in, const uint64_t *addend, uint64_t *out, int nl, uint32_t elt, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  return guarded([&] { return apply_galois_tail(c, in, {addend}, out, nl, elt, count, 1); });
}
int abc_hip_rotate_mac_plain(abc_hip_ctx *c, const uint64_t *in, const uint64_t *plain, size_t plain_stride, const uint64_t *addend,
                             uint64_t *out, int nl, int steps, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl) || check_mac_plain(c, "rotate_mac_plain", plain, plain_stride, plain_stride ? count : 1, out, count * 2 * (size_t)nl * c->n, nl)) return 1;
  return guarded([&] { return rotate_tail(c, in, {addend, plain, plain_stride}, out, nl, steps, count); });
}
int abc_hip_apply_galois_mac_plain(abc_hip_ctx *c, const uint64_t *in, const uint64_t *plain, size_t plain_stride, const uint64_t *addend,
                                   uint64_t *out, int nl, uint32_t elt, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl) || check_mac_plain(c, "apply_galois_mac_plain", plain, plain_stride, plain_stride ? count : 1, out, count * 2 * (size_t)nl * c->n, nl)) return 1;
  return guarded([&] { return apply_galois_tail(c, in, {addend, plain, plain_stride}, out, nl, elt, count, 1); });
}
int abc_hip_diag_matvec(abc_hip_ctx *c, const uint64_t *in, const uint64_t *diags, size_t diag_stride, const int *h_steps, int n_steps,
                        uint64_t *out, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (n_steps < 0 || (n_steps && !h_steps)) { set_error("diag_matvec: bad step list"); return 1; }
  if (diag_stride < (size_t)nl * c->n) { set_error("diag_matvec: diag_stride must be at least nl * N"); return 1; }
  if (check_mac_plain(c, "diag_matvec", diags, diag_stride, (size_t)n_steps, out, count * 2 * (size_t)nl * c->n, nl)) return 1;
  return guarded([&] { return diag_matvec(c, in, diags, diag_stride, std::vector<int>(h_steps, h_steps + n_steps), out, nl, count); });
}
int abc_hip_multiply_plain_sum(abc_hip_ctx *c, const uint64_t *const *h_ct, const uint64_t *const *h_plain, size_t plain_stride, int n_terms,
                               const uint64_t *addend, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  const char *op = "multiply_plain_sum";
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("multiply_plain_sum: CKKS only (a BFV plaintext product needs transforms)"); return 1; }
  if (check_level(c, nl) || check_plain_stride(c, op, plain_stride, nl)) return 1;
  if (size != 2 && size != 3) { set_error("multiply_plain_sum: size must be 2 or 3"); return 1; }
  if (n_terms < 0 || (n_terms && (!h_ct || !h_plain))) { set_error("multiply_plain_sum: bad term list"); return 1; }
  if (!out && count) { set_error("multiply_plain_sum: null output"); return 1; }
  const size_t pw = (size_t)nl * c->n, words = count * size * pw;
  for (int k = 0; k < n_terms; k++) {
    if (!h_ct[k] || !h_plain[k]) { set_error("multiply_plain_sum: null term pointer"); return 1; }
    if (words && ranges_overlap(h_ct[k], words * 8, out, words * 8)) { set_error("multiply_plain_sum: d_out must not overlap a ciphertext term"); return 1; }
    if (check_mac_plain(c, op, h_plain[k], plain_stride, plain_stride ? count : 1, out, words, nl)) return 1;
  }
  if (addend && addend != out && words && ranges_overlap(addend, words * 8, out, words * 8)) {
    set_error("multiply_plain_sum: d_out may be d_addend, but must not overlap it otherwise");
    return 1;
  }
  return guarded([&] {
    return plain_mac_sum(c, route_plain_mac_sum(c->facts, nl), std::vector<const u64 *>(h_ct, h_ct + n_terms),
                         std::vector<const u64 *>(h_plain, h_plain + n_terms), plain_stride, addend, out, size, nl, count);
  });
}
int abc_hip_rotate_plain(abc_hip_ctx *c, const uint64_t *plain, uint64_t *out, int nl, int steps, size_t rows) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("rotate_plain: CKKS only"); return 1; }
  if (check_level(c, nl)) return 1;
  const uint32_t elt = elt_from_step(c, steps);
  if (!elt) { set_error("step count too large"); return 1; }
  const size_t bytes = rows * (size_t)nl * c->n * 8;
  if (!bytes) return 0;
  if (ranges_overlap(plain, bytes, out, bytes)) { set_error("rotate_plain: d_out must not overlap d_plain"); return 1; }
  if (!steps) {
    ABC_HIP_CHECK(hipMemcpyAsync(out, plain, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  return launch_galois(c, plain, out, nl, rows, elt, true);
}
int abc_hip_diag_matvec_bsgs(abc_hip_ctx *c, const uint64_t *in, const uint64_t *diags, size_t diag_stride, const int *h_baby, int n_baby,
                             const int *h_giant, int n_giant, uint64_t *out, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if ((ptrdiff_t)count < 0) { set_error("diag_matvec_bsgs: negative count"); return 1; }
  if (n_baby < 0 || n_giant < 0 || (n_baby && !h_baby) || (n_giant && !h_giant)) { set_error("diag_matvec_bsgs: bad step list"); return 1; }
  if (diag_stride < (size_t)nl * c->n) { set_error("diag_matvec_bsgs: diag_stride must be at least nl * N"); return 1; }
  if (check_mac_plain(c, "diag_matvec_bsgs", diags, diag_stride, (size_t)n_baby * n_giant, out, count * 2 * (size_t)nl * c->n, nl)) return 1;
  return guarded([&] {
    return diag_matvec_bsgs(c, in, diags, diag_stride, std::vector<int>(h_baby, h_baby + n_baby), std::vector<int>(h_giant, h_giant + n_giant), out,
                            nl, count);
  });
}
int abc_hip_multiply_plain_sum_rescale(abc_hip_ctx *c, const uint64_t *const *h_ct, const uint64_t *const *h_plain, size_t plain_stride, int n_terms,
                                       const uint64_t *addend, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  const char *op = "multiply_plain_sum_rescale";
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("multiply_plain_sum_rescale is a CKKS operation"); return 1; }
  if (check_level(c, nl) || check_plain_stride(c, op, plain_stride, nl)) return 1;
  if (nl < 2) { set_error("multiply_plain_sum_rescale: no limb left to drop"); return 1; }
  if (size != 2 && size != 3) { set_error("multiply_plain_sum_rescale: size must be 2 or 3"); return 1; }
  if ((ptrdiff_t)count < 0) { set_error("multiply_plain_sum_rescale: negative count"); return 1; }
  if (n_terms < 0 || (n_terms && (!h_ct || !h_plain))) { set_error("multiply_plain_sum_rescale: bad term list"); return 1; }
  if (!out && count) { set_error("multiply_plain_sum_rescale: null output"); return 1; }
  const size_t N = (size_t)c->n, in_words = count * size * (size_t)nl * N, out_words = count * size * (size_t)(nl - 1) * N;
  for (int k = 0; k < n_terms; k++) {
    if (!h_ct[k] || !h_plain[k]) { set_error("multiply_plain_sum_rescale: null term pointer"); return 1; }
    if (out_words && ranges_overlap(h_ct[k], in_words * 8, out, out_words * 8)) { set_error("multiply_plain_sum_rescale: d_out must not overlap a ciphertext term (the output has one limb less per polynomial)"); return 1; }
    if (check_mac_plain(c, op, h_plain[k], plain_stride, plain_stride ? count : 1, out, out_words, nl)) return 1;
  }
  if (addend && out_words && ranges_overlap(addend, in_words * 8, out, out_words * 8)) {
    set_error("multiply_plain_sum_rescale: d_out must not overlap d_addend (the output has one limb less per polynomial)");
    return 1;
  }
  return guarded([&] {
    return plain_sum_rescale(c, std::vector<const u64 *>(h_ct, h_ct + n_terms), std::vector<const u64 *>(h_plain, h_plain + n_terms), plain_stride, addend,
                             out, size, nl, count);
  });
}
int abc_hip_diag_matvec_bsgs_rescale(abc_hip_ctx *c, const uint64_t *in, const uint64_t *diags, size_t diag_stride, const int *h_baby, int n_baby,
                                     const int *h_giant, int n_giant, uint64_t *out, int nl, size_t count) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("diag_matvec_bsgs_rescale is a CKKS operation"); return 1; }
  if (check_level(c, nl)) return 1;
  if (nl < 2) { set_error("diag_matvec_bsgs_rescale: no limb left to drop"); return 1; }
  if ((ptrdiff_t)count < 0) { set_error("diag_matvec_bsgs_rescale: negative count"); return 1; }
  if (n_baby < 0 || n_giant < 0 || (n_baby && !h_baby) || (n_giant && !h_giant)) { set_error("diag_matvec_bsgs_rescale: bad step list"); return 1; }
  if (diag_stride < (size_t)nl * c->n) { set_error("diag_matvec_bsgs_rescale: diag_stride must be at least nl * N"); return 1; }
  if (check_mac_plain(c, "diag_matvec_bsgs_rescale", diags, diag_stride, (size_t)n_baby * n_giant, out, count * 2 * (size_t)(nl - 1) * c->n, nl)) return 1;
  return guarded([&] {
    return diag_matvec_bsgs_rescale(c, in, diags, diag_stride, std::vector<int>(h_baby, h_baby + n_baby), std::vector<int>(h_giant, h_giant + n_giant),
                                    out, nl, count);
  });
}
int abc_hip_bfv_plain_to_ntt(abc_hip_ctx *c, const uint64_t *plain, uint64_t *plain_ntt, size_t rows) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_BFV) { set_error("bfv_plain_to_ntt: BFV only"); return 1; }
  if ((ptrdiff_t)rows < 0) { set_error("bfv_plain_to_ntt: negative row count"); return 1; }
  if (rows && (!plain || !plain_ntt)) { set_error("bfv_plain_to_ntt: null pointer"); return 1; }
  if (rows && ranges_overlap(plain, rows * c->n * 8, plain_ntt, rows * (size_t)c->L * c->n * 8)) { set_error("bfv_plain_to_ntt: d_plain_ntt must not overlap d_plain"); return 1; }
  return bfv_plain_to_ntt(c, plain, plain_ntt, rows);
}
int abc_hip_bfv_multiply_plain_sum(abc_hip_ctx *c, const uint64_t *const *h_ct, int ct_form, const uint64_t *const *h_plain_ntt,
                                   size_t plain_stride, int n_terms, const uint64_t *addend, uint64_t *out, int size, size_t count) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_BFV) { set_error("bfv_multiply_plain_sum: BFV only (CKKS: abc_hip_multiply_plain_sum)"); return 1; }
  if (size != 2 && size != 3) { set_error("bfv_multiply_plain_sum: size must be 2 or 3"); return 1; }
  const size_t pw = (size_t)c->L * c->n;
  if (plain_stride && plain_stride != pw) { set_error("bfv_multiply_plain_sum: plain_stride must be 0 or L * N"); return 1; }
  if (ct_form != ABC_HIP_CT_COEFF && ct_form != ABC_HIP_CT_NTT) { set_error("bfv_multiply_plain_sum: ct_form must be ABC_HIP_CT_COEFF or ABC_HIP_CT_NTT"); return 1; }
  if ((ptrdiff_t)count < 0) { set_error("bfv_multiply_plain_sum: negative count"); return 1; }
  if (n_terms < 0 || (n_terms && (!h_ct || !h_plain_ntt))) { set_error("bfv_multiply_plain_sum: bad term list"); return 1; }
  if (!out && count) { set_error("bfv_multiply_plain_sum: null output"); return 1; }
  const size_t words = count * size * pw, plain_words = count ? (plain_stride ? count * pw : pw) : 0;
  for (int k = 0; k < n_terms; k++) {
    if (!h_ct[k] || !h_plain_ntt[k]) { set_error("bfv_multiply_plain_sum: null term pointer"); return 1; }
    if (words && ranges_overlap(h_ct[k], words * 8, out, words * 8)) { set_error("bfv_multiply_plain_sum: d_out must not overlap a ciphertext term"); return 1; }
    if (words && ranges_overlap(h_plain_ntt[k], plain_words * 8, out, words * 8)) { set_error("bfv_multiply_plain_sum: the plaintext must not overlap d_out"); return 1; }
  }
  if (addend && addend != out && words && ranges_overlap(addend, words * 8, out, words * 8)) {
    set_error("bfv_multiply_plain_sum: d_out may be d_addend, but must not overlap it otherwise");
    return 1;
  }
  return guarded([&] { return bfv_multiply_plain_sum(c, h_ct, ct_form == ABC_HIP_CT_NTT, h_plain_ntt, plain_stride, n_terms, addend, out, size, count); });
}
int abc_hip_bfv_diag_matvec_bsgs(abc_hip_ctx *c, const uint64_t *in, const uint64_t *diags_ntt, size_t diag_stride, const int *h_baby, int n_baby,
                                 const int *h_giant, int n_giant, uint64_t *out, size_t count) {
  CTX_GUARD(c);
  const char *op = "bfv_diag_matvec_bsgs";
  if (c->scheme != ABC_HIP_SCHEME_BFV) { set_error(std::string(op) + ": BFV only (CKKS: abc_hip_diag_matvec_bsgs)"); return 1; }
  if ((ptrdiff_t)count < 0) { set_error(std::string(op) + ": negative count"); return 1; }
  if (n_baby < 0 || n_giant < 0 || (n_baby && !h_baby) || (n_giant && !h_giant)) { set_error(std::string(op) + ": bad step list"); return 1; }
  const size_t pw = (size_t)c->L * c->n, rows = (size_t)n_baby * n_giant, out_words = count * 2 * pw;
  if (diag_stride < pw) { set_error(std::string(op) + ": diag_stride must be at least L * N"); return 1; }
  if (count && (!in || !out || (rows && !diags_ntt))) { set_error(std::string(op) + ": null pointer"); return 1; }
  if (rows && out_words && ranges_overlap(diags_ntt, ((rows - 1) * diag_stride + pw) * 8, out, out_words * 8)) { set_error(std::string(op) + ": the plaintext must not overlap d_out"); return 1; }
  return guarded([&] {
    return diag_matvec_bsgs(c, in, diags_ntt, diag_stride, std::vector<int>(h_baby, h_baby + n_baby), std::vector<int>(h_giant, h_giant + n_giant), out,
                            c->L, count);
  });
}
int abc_hip_rotate_sum(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int nl, const int *h_steps, int n_steps, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (n_steps < 0 || (n_steps && !h_steps)) { set_error("rotate_sum: bad step list"); return 1; }
  return guarded([&] { return rotate_sum(c, in, out, nl, std::vector<int>(h_steps, h_steps + n_steps), count); });
}
int abc_hip_apply_galois_hoisted(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int nl, const uint32_t *h_elts, int n_elts,
                                 size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (n_elts < 0 || (n_elts && !h_elts)) { set_error("apply_galois_hoisted: bad element list"); return 1; }
  for (int r = 0; r < n_elts; r++)
    if (!(h_elts[r] & 1) || h_elts[r] >= 2u * (uint32_t)c->n) { set_error("Galois element must be odd and below 2N"); return 1; }
  return guarded([&] { return hoisted(c, in, out, nl, std::vector<uint32_t>(h_elts, h_elts + n_elts), count); });
}
int abc_hip_rotate_hoisted(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int nl, const int *h_steps, int n_steps, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  if (n_steps < 0 || (n_steps && !h_steps)) { set_error("rotate_hoisted: bad step list"); return 1; }
  std::vector<uint32_t> elts((size_t)n_steps, 0);
  for (int r = 0; r < n_steps; r++) {
    if (!h_steps[r]) continue;  // a copy
    if (!(elts[r] = elt_from_step(c, h_steps[r]))) { set_error("step count too large"); return 1; }
  }
  return guarded([&] { return hoisted(c, in, out, nl, elts, count); });
}
int abc_hip_multiply_plain(abc_hip_ctx *c, const uint64_t *ct, const uint64_t *plain, size_t plain_stride, uint64_t *out, int size,
                           int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl) || check_plain_stride(c, "multiply_plain", plain_stride, nl)) return 1;
  if (c->scheme == ABC_HIP_SCHEME_CKKS) return ckks_multiply_plain(c, ct, plain, plain_stride, out, size, nl, count);
  return bfv_multiply_plain(c, ct, plain, plain_stride, out, size, count);
}
int abc_hip_add_plain(abc_hip_ctx *c, const uint64_t *ct, const uint64_t *plain, size_t plain_stride, uint64_t *out, int size, int nl,
                      size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl) || check_plain_stride(c, "add_plain", plain_stride, nl)) return 1;
  if (c->scheme == ABC_HIP_SCHEME_CKKS) return ckks_add_plain(c, ct, plain, plain_stride, out, size, nl, count, 0);
  return bfv_addsub_plain(c, ct, plain, plain_stride, out, size, count, 0);
}
int abc_hip_sub_plain(abc_hip_ctx *c, const uint64_t *ct, const uint64_t *plain, size_t plain_stride, uint64_t *out, int size, int nl,
                      size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl) || check_plain_stride(c, "sub_plain", plain_stride, nl)) return 1;
  if (c->scheme == ABC_HIP_SCHEME_CKKS) return ckks_add_plain(c, ct, plain, plain_stride, out, size, nl, count, 1);
  return bfv_addsub_plain(c, ct, plain, plain_stride, out, size, count, 1);
}
int abc_hip_rescale(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("rescale is a CKKS operation"); return 1; }
  if (check_level(c, nl)) return 1;
  if (in == out) { set_error("rescale: d_out must not alias d_in (the output has one limb less per polynomial)"); return 1; }
  return launch_rescale(c, in, out, size, nl, count);
}
int abc_hip_multiply_plain_rescale(abc_hip_ctx *c, const uint64_t *ct, const uint64_t *plain, size_t plain_stride, uint64_t *out, int size,
                                   int nl, size_t count) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("multiply_plain_rescale is a CKKS operation"); return 1; }
  if (check_level(c, nl)) return 1;
  if (nl < 2) { set_error("multiply_plain_rescale: no limb left to drop"); return 1; }
  if (size != 2 && size != 3) { set_error("multiply_plain_rescale: size must be 2 or 3"); return 1; }
  const size_t N = (size_t)c->n, out_words = count * size * (size_t)(nl - 1) * N;
  if (check_mac_plain(c, "multiply_plain_rescale", plain, plain_stride, plain_stride ? count : 1, out, out_words, nl)) return 1;
  if (out_words && ranges_overlap(ct, count * size * (size_t)nl * N * 8, out, out_words * 8)) {
    set_error("multiply_plain_rescale: d_out must not overlap d_ct (the output has one limb less per polynomial)");
    return 1;
  }
  return launch_mulplain_rescale(c, ct, plain, plain_stride, out, size, nl, count);
}
int abc_hip_mod_switch(abc_hip_ctx *c, const uint64_t *in, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("mod_switch is only implemented for CKKS"); return 1; }
  if (check_level(c, nl)) return 1;
  if (in == out) { set_error("mod_switch: d_out must not alias d_in (the output has one limb less per polynomial)"); return 1; }
  return launch_drop_last(c, in, out, size, nl, count);
}

// ---- scalar constants and polynomial evaluation (CKKS) ----
int abc_hip_ckks_const_words(abc_hip_ctx *c, double value, double scale, int nl, uint64_t *h_words) {
  if (!c) { set_error("null context"); return 1; }
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("ckks_const_words is a CKKS operation"); return 1; }
  if (nl < 1 || nl > c->L) { set_error("limb count out of range for this context"); return 1; }
  if (!h_words) { set_error("ckks_const_words: null output"); return 1; }
  u64 w[kMaxLimbs];
  if (const_words(c, "ckks_const_words", value, scale, nl, w)) return 1;  // nothing written on failure
  std::memcpy(h_words, w, (size_t)nl * 8);
  return 0;
}
// what both scalar-weighted sums check before anything is written or enqueued; out_nl: nl, or nl - 1 for the rescaled form, where
// d_out may not even BE d_addend (the shapes differ)
static int check_const_sum(abc_hip_ctx *c, const std::string &op, const uint64_t *const *h_ct, const int *h_ct_nl, const uint64_t *h_weights, int n_terms,
                           const uint64_t *h_const, const uint64_t *addend, const uint64_t *out, int size, int nl, int out_nl, size_t count) {
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error(op + " is a CKKS operation"); return 1; }
  if (check_level(c, nl)) return 1;
  if (out_nl < 1) { set_error(op + ": no limb left to drop"); return 1; }
  if (size != 2 && size != 3) { set_error(op + ": size must be 2 or 3"); return 1; }
  if ((ptrdiff_t)count < 0) { set_error(op + ": negative count"); return 1; }
  if (n_terms < 0 || (n_terms && (!h_ct || !h_weights))) { set_error(op + ": bad term list"); return 1; }
  if (!out && count) { set_error(op + ": null output"); return 1; }
  const size_t N = (size_t)c->n, out_bytes = count * size * (size_t)out_nl * N * 8;
  for (int k = 0; k < n_terms; k++) {
    if (!h_ct[k]) { set_error(op + ": null term pointer"); return 1; }
    const int l = h_ct_nl ? h_ct_nl[k] : nl;
    if (l < nl || l > c->L) { set_error(op + ": a term's limb count must be in nl .. L"); return 1; }
    for (int j = 0; j < nl; j++)
      if (h_weights[(size_t)k * nl + j] >= c->primes[j]) { set_error(op + ": a weight word is not below its prime"); return 1; }
    if (out_bytes && ranges_overlap(h_ct[k], count * size * (size_t)l * N * 8, out, out_bytes)) { set_error(op + ": d_out must not overlap a ciphertext term"); return 1; }
  }
  for (int j = 0; h_const && j < nl; j++)
    if (h_const[j] >= c->primes[j]) { set_error(op + ": a constant word is not below its prime"); return 1; }
  if (addend && !(out_nl == nl && addend == out) && out_bytes && ranges_overlap(addend, count * size * (size_t)nl * N * 8, out, out_bytes)) {
    set_error(op + (out_nl == nl ? ": d_out may be d_addend, but must not overlap it otherwise" : ": d_out must not overlap d_addend (the output has one limb less per polynomial)"));
    return 1;
  }
  return 0;
}
static std::vector<int> term_levels(const int *h_ct_nl, int n_terms, int nl) {
  std::vector<int> v((size_t)n_terms, nl);
  for (int k = 0; h_ct_nl && k < n_terms; k++) v[k] = h_ct_nl[k];
  return v;
}
int abc_hip_multiply_const_sum(abc_hip_ctx *c, const uint64_t *const *h_ct, const int *h_ct_nl, const uint64_t *h_weights, int n_terms,
                               const uint64_t *h_const, const uint64_t *addend, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_const_sum(c, "multiply_const_sum", h_ct, h_ct_nl, h_weights, n_terms, h_const, addend, out, size, nl, nl, count)) return 1;
  return guarded([&] {
    return const_mac_sum(c, route_const_mac_sum(c->facts, nl), std::vector<const u64 *>(h_ct, h_ct + n_terms), term_levels(h_ct_nl, n_terms, nl), h_weights,
                         h_const, addend, out, size, nl, count);
  });
}
int abc_hip_multiply_const_sum_rescale(abc_hip_ctx *c, const uint64_t *const *h_ct, const int *h_ct_nl, const uint64_t *h_weights, int n_terms,
                                       const uint64_t *h_const, const uint64_t *addend, uint64_t *out, int size, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_const_sum(c, "multiply_const_sum_rescale", h_ct, h_ct_nl, h_weights, n_terms, h_const, addend, out, size, nl, nl - 1, count)) return 1;
  return guarded([&] {
    return const_sum_rescale(c, std::vector<const u64 *>(h_ct, h_ct + n_terms), term_levels(h_ct_nl, n_terms, nl), h_weights, h_const, addend, out, size,
                             nl, count);
  });
}

static int ceil_log2(int k) {  // k >= 1
  int e = 0;
  while ((1 << e) < k) e++;
  return e;
}
int abc_hip_ckks_poly_eval_depth(int degree) {
  if (degree < 1) { set_error("ckks_poly_eval_depth: degree must be at least 1"); return -1; }
  return ceil_log2(degree) + 1;
}
// The fixed sequence of abc_hip.h.  Everything a refusal depends on -- the levels, the scales, every weight -- is worked out on
// the host before the first launch.  Per group of ciphertexts (arena_group: the POWERS, arena 5, stay within 4 GiB; the lowered factor,
// the product and the last step's sum -- arenas 3, 4 and 1 -- are one ciphertext of at most nl limbs per member of the group each): power k, ascending, is
// mul_relin of x^h and x^l at nl - e + 1 limbs -- x^l lowered into arena 3 where it is held higher -- into arena 4, then the
// rescale into the power's slab of arena 5; the last step is const_sum_rescale over x (in place in d_x) and the slabs, each read at
// its own level (arenas 1, 2, 6).
static int poly_eval(abc_hip_ctx *c, const u64 *x, double x_scale, const double *coeffs, int degree, double out_scale, u64 *out, int nl, size_t count) {
  const int d = degree, E = ceil_log2(d), m = nl - E;
  const size_t N = (size_t)c->n;
  std::vector<int> level(d + 1, nl), hi(d + 1, 0), lo(d + 1, 0);
  std::vector<double> scale(d + 1, x_scale);
  std::vector<char> need(d + 1, 0);
  for (int k = 2; k <= d; k++) {
    const int e = ceil_log2(k);
    hi[k] = 1 << (e - 1), lo[k] = k - hi[k], level[k] = nl - e;
    scale[k] = scale[hi[k]] * scale[lo[k]] / (double)c->primes[nl - e];
  }
  for (int k = 1; k <= d; k++) need[k] = coeffs[k] != 0.0;
  for (int k = d; k >= 2; k--)
    if (need[k]) need[hi[k]] = need[lo[k]] = 1;
  const double top = out_scale * (double)c->primes[m - 1];
  std::vector<int> terms;  // the powers with a non-zero coefficient: a zero weight adds nothing to any word
  for (int k = 1; k <= d; k++)
    if (coeffs[k] != 0.0) terms.push_back(k);
  std::vector<u64> w(terms.size() * (size_t)m + 1), w0(m);
  for (size_t i = 0; i < terms.size(); i++)
    if (const_words(c, "ckks_poly_eval", coeffs[terms[i]], top / scale[terms[i]], m, w.data() + i * m)) return 1;
  if (const_words(c, "ckks_poly_eval", coeffs[0], top, m, w0.data())) return 1;
  if (!count) return 0;
  size_t slab_limbs = 0;  // limbs per ciphertext polynomial pair over the powers kept
  std::vector<size_t> slab_at(d + 1, 0);
  int kept = 0;
  for (int k = 2; k <= d; k++)
    if (need[k]) slab_at[k] = slab_limbs, slab_limbs += (size_t)level[k], kept++;
  const size_t group = arena_group(c->facts, nl, count, 2 * (size_t)(kept ? kept : 1));
  if (kept && (ensure_aux(c, 5, group * 2 * slab_limbs * N * 8) || ensure_aux(c, 3, group * 2 * (size_t)nl * N * 8) || ensure_aux(c, 4, group * 2 * (size_t)nl * N * 8))) return 1;
  std::vector<const u64 *> ct(terms.size());
  std::vector<int> ct_nl(terms.size());
  for (size_t off = 0; off < count; off += group) {
    const size_t cc = count - off < group ? count - off : group;
    const u64 *gx = x + off * 2 * (size_t)nl * N;
    auto power = [&](int k) -> u64 * { return k == 1 ? const_cast<u64 *>(gx) : (u64 *)c->aux[5] + group * 2 * slab_at[k] * N; };
    for (int k = 2; k <= d; k++) {
      if (!need[k]) continue;
      const int lk = level[k] + 1;  // the product's level: that of x^h
      const u64 *a = power(hi[k]), *b = power(lo[k]);
      if (level[lo[k]] > lk) {
        if (launch_drop_to(c, b, (u64 *)c->aux[3], level[lo[k]], lk, cc * 2)) return 1;
        b = (const u64 *)c->aux[3];
      }
      if (mul_relin(c, a, b, (u64 *)c->aux[4], lk, cc)) return 1;
      if (launch_rescale(c, (const u64 *)c->aux[4], power(k), 2, lk, cc)) return 1;
    }
    for (size_t i = 0; i < terms.size(); i++) ct[i] = power(terms[i]), ct_nl[i] = level[terms[i]];
    if (const_sum_rescale(c, ct, ct_nl, w.data(), w0.data(), nullptr, out + off * 2 * (size_t)(m - 1) * N, 2, m, cc)) return 1;
  }
  return 0;
}
int abc_hip_ckks_poly_eval(abc_hip_ctx *c, const uint64_t *d_x, double x_scale, const double *h_coeffs, int degree, double out_scale, uint64_t *d_out,
                           int nl, size_t count) {
  CTX_GUARD(c);
  if (c->scheme != ABC_HIP_SCHEME_CKKS) { set_error("ckks_poly_eval is a CKKS operation"); return 1; }
  if (check_level(c, nl)) return 1;
  if (degree < 1 || degree > 31) { set_error("ckks_poly_eval: degree must be in 1 .. 31"); return 1; }
  const int depth = ceil_log2(degree) + 1;
  if (nl < depth + 1) { set_error("ckks_poly_eval: the chain is too short (nl must be at least ceil(log2 degree) + 2)"); return 1; }
  if ((ptrdiff_t)count < 0) { set_error("ckks_poly_eval: negative count"); return 1; }
  if (!h_coeffs) { set_error("ckks_poly_eval: null coefficients"); return 1; }
  if (!std::isfinite(x_scale) || !std::isfinite(out_scale) || x_scale <= 0 || out_scale <= 0) { set_error("ckks_poly_eval: scales must be finite and positive"); return 1; }
  for (int k = 0; k <= degree; k++)
    if (!std::isfinite(h_coeffs[k])) { set_error("ckks_poly_eval: a coefficient is not finite"); return 1; }
  if (!c->d_relin) { set_error("ckks_poly_eval: no relinearisation key"); return 1; }
  if (count && (!d_x || !d_out)) { set_error("ckks_poly_eval: null ciphertext pointer"); return 1; }
  const size_t N = (size_t)c->n;
  if (count && ranges_overlap(d_x, count * 2 * (size_t)nl * N * 8, d_out, count * 2 * (size_t)(nl - depth) * N * 8)) {
    set_error("ckks_poly_eval: d_out must not overlap d_x");
    return 1;
  }
  return guarded([&] { return poly_eval(c, d_x, x_scale, h_coeffs, degree, out_scale, d_out, nl, count); });
}

// ---- raw pieces ----
static int ntt_entry(abc_hip_ctx *c, uint64_t *d, int kind, int index, size_t count, bool fwd) {
  int mid;
  if (kind == 0) {
    if (index < 0 || index >= c->K) { set_error("ntt: prime index out of range"); return 1; }
    mid = index;
  } else if (kind == 1) {
    if (c->scheme != ABC_HIP_SCHEME_BFV || index < 0 || index >= c->nBsk) { set_error("ntt: Bsk index out of range"); return 1; }
    mid = c->dc.id_bsk + index;
  } else if (kind == 2) {
    if (c->scheme != ABC_HIP_SCHEME_BFV) { set_error("ntt: no plaintext modulus in a CKKS context"); return 1; }
    mid = c->dc.id_t;
  } else {
    set_error("ntt: bad modulus kind");
    return 1;
  }
  LimbMap map{};
  map.id[0] = mid;
  return fwd ? launch_ntt_fwd(c, d, map, 1, count) : launch_ntt_inv(c, d, map, 1, count);
}
int abc_hip_ntt_forward(abc_hip_ctx *c, uint64_t *d, int kind, int index, size_t count) { CTX_GUARD(c); return ntt_entry(c, d, kind, index, count, true); }
int abc_hip_ntt_inverse(abc_hip_ctx *c, uint64_t *d, int kind, int index, size_t count) { CTX_GUARD(c); return ntt_entry(c, d, kind, index, count, false); }

int abc_hip_ntt_limbs(abc_hip_ctx *c, uint64_t *d, int nl, size_t polys, int inverse) {
  CTX_GUARD(c);
  if (nl < 1 || nl > c->L) { set_error("ntt_limbs: limb count out of range"); return 1; }
  const LimbMap map = key_limb_map(c, nl);
  return inverse ? launch_ntt_inv(c, d, map, nl, polys * nl) : launch_ntt_fwd(c, d, map, nl, polys * nl);
}

int abc_hip_keyswitch(abc_hip_ctx *c, const uint64_t *target, uint32_t key_kind, uint64_t *out2, int nl, size_t count) {
  CTX_GUARD(c);
  if (check_level(c, nl)) return 1;
  const uint64_t *key = nullptr;
  if (key_kind == 0) key = c->d_relin;
  else if (c->d_galois.count(key_kind)) key = c->d_galois[key_kind];
  if (!key) { set_error("keyswitch: key not present"); return 1; }
  KsOperands o;  // one polynomial per ciphertext, no addend
  o.target = target, o.target_stride = (size_t)nl * c->n, o.key = key, o.out = out2, o.nl = nl, o.count = count;
  return launch_keyswitch(c, route_keyswitch(c->facts, nl), o);
}

// ---- graph capture ----
int abc_hip_graph_begin(abc_hip_ctx *c) { CTX_GUARD(c); return graph_begin(c); }
int abc_hip_graph_end(abc_hip_ctx *c, void **out) { CTX_GUARD(c); return graph_end(c, out); }
int abc_hip_graph_launch(abc_hip_ctx *c, void *exec) {
  CTX_GUARD(c);
  ABC_HIP_CHECK(hipGraphLaunch((hipGraphExec_t)exec, c->stream));
  return 0;
}
int abc_hip_graph_destroy(abc_hip_ctx *c, void *exec) { CTX_GUARD(c); return graph_destroy(c, exec); }

int abc_hip_microbench(abc_hip_ctx *c, int which, int iters, double *ms) { CTX_GUARD(c); return microbench(c, which, iters, ms); }

int abc_hip_timer_start(abc_hip_ctx *c) {
  CTX_GUARD(c);
  ABC_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
  return 0;
}
int abc_hip_timer_stop(abc_hip_ctx *c, float *ms) {
  CTX_GUARD(c);
  ABC_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
  ABC_HIP_CHECK(hipEventSynchronize(c->ev1));
  ABC_HIP_CHECK(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return 0;
}

}  // extern "C"
