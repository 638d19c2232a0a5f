// abc_context.hpp -- host-side context of libabc_hip.so and the structs shared with device code.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "abc_buffers.hpp"
#include "abc_modarith.hpp"
#include "abc_ntt.hpp"
#include "abc_route.hpp"

namespace abc {

constexpr int kMaxLimbs = 16;

// limb index -> modulus id (index into DevCtx::mods / twiddle tables)
struct LimbMap {
  int id[kMaxLimbs + 1];
};

// small read-only constants, one instance per context in device memory
struct DevConst {
  // key switching / modulus switching
  u64 inv_special[kMaxLimbs], inv_special_s[kMaxLimbs];        // q_special^-1 mod q_j (+Shoup)
  u64 inv_qlast[kMaxLimbs][kMaxLimbs], inv_qlast_s[kMaxLimbs][kMaxLimbs];  // [l][j] = q_l^-1 mod q_j
  u64 special_mod_q[kMaxLimbs], special_mod_q_s[kMaxLimbs];
  double inv_special_c[kMaxLimbs], inv_special_cq[kMaxLimbs];  // fp64 path: centred value and value / q_j
  double special_c[kMaxLimbs], special_cq[kMaxLimbs];          // q_special mod q_j, centred, and that / q_j
  double inv_qlast_c[kMaxLimbs][kMaxLimbs], inv_qlast_cq[kMaxLimbs][kMaxLimbs];  // same for inv_qlast (rescale)                                // q_special mod q_j (key generation)
  // BFV plaintext scaling (Evaluator::add_plain / Encryptor)
  u64 q_mod_t, upper_half_threshold, t;
  u64 coeff_div_plain[kMaxLimbs], upper_half_increment[kMaxLimbs];
  // BEHZ
  int nq, nB, nBsk, pad_;
  u64 mtilde_mod_q[kMaxLimbs];
  u64 inv_punct_q[kMaxLimbs];
  u64 q_to_bsk[kMaxLimbs][kMaxLimbs];  // [j][i] (q/q_i) mod Bsk_j
  u64 q_to_mtilde[kMaxLimbs];          // (q/q_i) mod 2^32
  u64 neg_inv_q_mod_mtilde;
  u64 q_mod_bsk[kMaxLimbs], inv_mtilde_mod_bsk[kMaxLimbs], inv_q_mod_bsk[kMaxLimbs];
  u64 inv_punct_B[kMaxLimbs];
  u64 B_to_q[kMaxLimbs][kMaxLimbs];  // [i][b] (B/B_b) mod q_i
  u64 B_to_msk[kMaxLimbs];
  u64 inv_B_mod_msk, B_mod_q[kMaxLimbs];
  u64 t_mod_q[kMaxLimbs], t_mod_bsk[kMaxLimbs];
  // fused constants with Shoup quotients (a constant operand costs half a Barrett multiply):
  u64 ext_q[kMaxLimbs], ext_q_s[kMaxLimbs];          // m~ * (q/q_i)^-1 mod q_i          (BEHZ extend)
  u64 flr_q[kMaxLimbs], flr_q_s[kMaxLimbs];          // t  * (q/q_i)^-1 mod q_i          (BEHZ floor)
  u64 tinvq_bsk[kMaxLimbs], tinvq_bsk_s[kMaxLimbs];  // t * q^-1 mod Bsk_j
  u64 inv_q_mod_bsk_s[kMaxLimbs], inv_mtilde_mod_bsk_s[kMaxLimbs], inv_punct_B_s[kMaxLimbs];
  u64 inv_B_mod_msk_s, B_mod_q_s[kMaxLimbs];
  u64 dec_q[kMaxLimbs], dec_q_s[kMaxLimbs];          // t*gamma * (q/q_i)^-1 mod q_i     (decrypt)
  // Shoup quotients of the base-conversion matrices (lazy dot products: one mulhi per term, no 128-bit sums)
  u64 q_to_bsk_s[kMaxLimbs][kMaxLimbs], B_to_q_s[kMaxLimbs][kMaxLimbs], B_to_msk_s[kMaxLimbs], q_mod_bsk_s[kMaxLimbs];
  // BFV decryption (decrypt_scale_and_round)
  u64 tgamma_mod_q[kMaxLimbs], q_to_t[kMaxLimbs], q_to_gamma[kMaxLimbs];
  u64 neg_inv_q_mod_t, neg_inv_q_mod_gamma, inv_gamma_mod_t, gamma;
};

// fp64 twins of the BEHZ constants ({value centred into (-p/2, p/2], value / p}: the operand pair of fp_mul_lazy), filled
// when every ciphertext prime and every auxiliary prime is below 2^50 (abc_kernels_bfv.hip, k_behz_extend_fp / k_behz_floor_fp)
struct DevConstFp {
  double ext_q[kMaxLimbs][2], flr_q[kMaxLimbs][2], B_mod_q[kMaxLimbs][2];
  double q_to_bsk[kMaxLimbs][kMaxLimbs][2];  // [j][i]
  double B_to_q[kMaxLimbs][kMaxLimbs][2];    // [i][b]
  double q_mod_bsk[kMaxLimbs][2], inv_mtilde_mod_bsk[kMaxLimbs][2], tinvq_bsk[kMaxLimbs][2], inv_q_mod_bsk[kMaxLimbs][2];
  double inv_punct_B[kMaxLimbs][2], B_to_msk[kMaxLimbs][2], inv_B_mod_msk[2];
};

// passed BY VALUE to every kernel
struct DevCtx {
  const Mod *mods;      // [nmods]
  const u64 *tw;        // [nmods][2][N][2]: forward {w, Shoup} pairs, then inverse pairs
  const double *ftw;    // [nmods][2][N]: fp64 twin, w centred (one double per twiddle), forward then inverse; primes < 2^50 only
  const DevConst *cst;  //
  const DevConstFp *cstf;  // null unless the BEHZ base is fp64-capable
  const u32 *slot_map;  // [N] BatchEncoder index map (BFV)
  int logn, n;
  int ps;               // scratch limb stride of the split kernels in words (always n)
  int K, L;             // key-level primes, data limbs
  int id_bsk, id_t, id_gamma, id_mtilde;  // modulus ids: key primes are 0..K-1
};

__device__ __forceinline__ NttTable ntt_table(const DevCtx &c, int mid) {
  const u64 *b = c.tw + (size_t)mid * 4 * c.n;
  NttTable t;
  t.tw = reinterpret_cast<const u64x2 *>(b);
  t.itw = reinterpret_cast<const u64x2 *>(b + 2 * (size_t)c.n);
  return t;
}

// modulus constants through the constant address space (scalar loads wherever the id is wave-uniform; see FpTable)
__device__ __forceinline__ Mod mod_at(const DevCtx &c, int id) {
  const ABC_CONST_AS Mod *p = (const ABC_CONST_AS Mod *)(c.mods + id);
  Mod m;
  m.q = p->q; m.mu = p->mu; m.two_q = p->two_q; m.shift = p->shift; m.bits = p->bits;
  m.inv_n = p->inv_n; m.inv_n_s = p->inv_n_s; m.qd = p->qd; m.qinv = p->qinv;
  m.inv_n_c = p->inv_n_c; m.inv_n_cq = p->inv_n_cq;
  return m;
}
__device__ __forceinline__ FpTable fp_table(const DevCtx &c, int mid) {
  const double *b = c.ftw + (size_t)mid * 2 * c.n;
  FpTable t;
  t.tw = (const ABC_CONST_AS double *)(b);
  t.itw = (const ABC_CONST_AS double *)(b + (size_t)c.n);
  return t;
}
// modulus constants and twiddle table of an arithmetic policy (abc_ntt.hpp), each fetched the way its kernels always did
template <class A>
__device__ __forceinline__ Mod arith_mod(const DevCtx &c, int id) {
  if constexpr (std::is_same_v<typename A::E, double>) return mod_at(c, id);
  else return c.mods[id];
}
template <class A>
__device__ __forceinline__ typename A::Table arith_table(const DevCtx &c, int mid) {
  if constexpr (std::is_same_v<typename A::E, double>) return fp_table(c, mid);
  else return ntt_table(c, mid);
}
// p^-1 mod q_j for the two dropped primes there are: the special prime (key-switch mod-down), limb l = nl - 1 (rescale)
__device__ __forceinline__ DropInv inv_special_at(const DevCtx &c, int j) {
  return DropInv{c.cst->inv_special[j], c.cst->inv_special_s[j], c.cst->inv_special_c[j], c.cst->inv_special_cq[j]};
}
__device__ __forceinline__ DropInv inv_qlast_at(const DevCtx &c, int l, int j) {
  return DropInv{c.cst->inv_qlast[l][j], c.cst->inv_qlast_s[l][j], c.cst->inv_qlast_c[l][j], c.cst->inv_qlast_cq[l][j]};
}
// The `members` workgroups that read one shared polynomial are 8 apart in blockIdx: workgroups go round-robin over the 8 XCDs,
// so they share one L2 and the polynomial is fetched from HBM once, not `members` times.  Polynomials are taken eight at a time;
// the last group may be ragged.  -> member j of polynomial p
__device__ __forceinline__ void xcd_slot(unsigned bid, int members, int npoly, int &j, size_t &p) {
  const unsigned per = 8u * (unsigned)members;
  const unsigned grp = bid / per, rem = bid % per;
  const unsigned left = (unsigned)npoly - grp * 8u, gsz = left < 8u ? left : 8u;
  j = (int)(rem / gsz);
  p = (size_t)grp * 8 + rem % gsz;
}

}  // namespace abc

// The opaque C-ABI handle.
struct abc_hip_ctx {
  int scheme = 0, logn = 0, n = 0, K = 0, L = 0, device = 0;
  std::vector<uint64_t> primes;  // key-level chain: data limbs + special
  uint64_t t = 0;
  hipStream_t stream = nullptr;      // stream every operation is enqueued on
  hipStream_t own_stream = nullptr;  // the context's private stream (default)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // two internal lanes let an HBM-streaming kernel of one chunk overlap an ALU-bound transform of another
  static constexpr int kMaxLanes = 4;
  hipStream_t lane[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t lane_fork = nullptr, lane_join[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
  // moduli: ids 0..K-1 key primes, then Bsk (B_0..B_{nB-1}, m_sk), gamma, t, m_tilde(arith only)
  std::vector<abc::Mod> h_mods;
  std::vector<uint64_t> mod_values;
  int nB = 0, nBsk = 0;
  abc::DevCtx dc{};
  abc::DevConst h_cst{};
  abc::Mod *d_mods = nullptr;
  uint64_t *d_tw = nullptr;
  double *d_ftw = nullptr;
  // Every device buffer a recorded circuit (abc_hip_graph_*) may have baked into its kernel arguments -- abc_hip_malloc blocks,
  // workspace, arenas, keys, key mirrors -- and the graphs that own it: one table, one rule (abc_buffers.hpp), driven by
  // abc_buffers.hip.  cache_alloc: abc_hip_free recycles blocks through the table's cache (off: ABC_HIP_SYNC_ALLOC=1).
  bool cache_alloc = false;
  // ABC_HIP_POISON=1 (debug, read when the context is created): every block abc_hip_malloc hands out, and the scratch arenas when
  // they grow and when an outermost C-ABI operation begins (op_depth: a composite call that re-enters the C ABI keeps its
  // intermediate state), are filled with 0xFF bytes -- no residue as a u64, a NaN as a double (abc_buffers.hip)
  bool poison = false;
  std::atomic<int> op_depth{0};
  mutable std::mutex alloc_mu;  // guards `buffers`
  abc::BufferTable buffers;
  bool behz_fp = false;  // BFV: 50-bit BEHZ auxiliary base and fp64 base-conversion kernels
  bool use_fp = true;  // fp64 transforms for primes < 2^50 (ABC_HIP_NO_FP64=1 forces the integer path)
  // Path switches and everything else a kernel sequence is chosen by (abc_route.hpp): filled ONCE, when the context is created
  // (abc_hip_ctx_reload_env fills them again), never on the per-operation path.
  using Switches = abc::Switches;
  Switches sw;
  abc::RouteFacts facts;
  abc::DevConst *d_cst = nullptr;
  abc::DevConstFp *d_cstf = nullptr;
  uint32_t *d_slot_map = nullptr;
  void *d_ckks_codec = nullptr;  // CKKS slot codec tables (twiddles, twist, slot map), built on first use
  void *d_crt = nullptr;         // CRT constants of the exact centred lift (abc_crt_lift.hpp), either scheme, built on first use
  // keys (device)
  uint64_t *d_sk = nullptr, *d_pk = nullptr, *d_relin = nullptr;
  std::map<uint32_t, uint64_t *> d_galois;
  // mirrors of key-switching keys (fp64 twin: centred doubles; Shoup quotients; same layout), built on first use, rebuilt in place
  // when the key they mirror is rewritten (abc_buffers.hip).  perm: the Galois key with every [N] row permuted by the inverse
  // element perm_ginv (hoisted rotations); it is a key-switching key itself and has an entry, and so mirrors, of its own.
  struct KeyMirror {
    double *twin = nullptr;
    uint64_t *shoup = nullptr;
    uint64_t *perm = nullptr;
    uint32_t perm_ginv = 0;
  };
  std::unordered_map<const uint64_t *, KeyMirror> key_mirrors;
  std::vector<uint32_t> galois_order;
  // workspace (kernel-sequence scratch) and seven caller-level arenas (0: permuted input, 1 / 2: products (multiply_plain_rescale's separate route and multiply_plain_sum_rescale's leading sum among them) and rotation ping-pong, 3 / 4: rotate_sum's running sums
  // and poly_eval's lowered factor and product, 5: poly_eval's powers, 6: the constant plaintext and lowered term of multiply_const_sum's composed route);
  // all grow on demand and are reused, so steady-state calls perform no hipMalloc / hipFree; one that grows while a graph owns
  // it is held back, not freed (ensure_arena in abc_buffers.hip)
  void *ws = nullptr;
  size_t ws_bytes = 0;
  void *aux[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t aux_bytes[7] = {0, 0, 0, 0, 0, 0, 0};
  size_t limb_words() const { return (size_t)n; }
  size_t key_words() const { return (size_t)L * 2 * K * n; }
};

namespace abc {

void set_error(const std::string &msg);
#define ABC_HIP_CHECK(expr)                                                                         \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      abc::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                            \
      return 1;                                                                                     \
    }                                                                                               \
  } while (0)

// grid of a grid-stride kernel over `items`: enough workgroups to fill 256 CUs several times, the stride loop beyond
inline unsigned grid_for(size_t items, int block) {
  size_t g = (items + block - 1) / block;
  const size_t cap = 256 * 8 * 4;
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}
// Host-synchronising entry points cannot be recorded, and letting HIP find that out invalidates the capture for good on this
// runtime (the stream keeps returning hipErrorStreamCaptureInvalidated even after hipStreamEndCapture): refuse up front.
#define NOT_CAPTURABLE(c, what)                                                                                   \
  do {                                                                                                            \
    if ((c)->buffers.capturing) { abc::set_error(what ": not capturable (host transfer / synchronisation inside abc_hip_graph_begin..end)"); return 1; } \
  } while (0)

// One key switch as every layer from the C ABI to the launch passes it on: out[ct] = KeySwitch(target[ct]) (+ addend[ct]) (+ acc[ct]),
// or acc[ct] + plain[ct] (.) (KeySwitch(target[ct]) + addend[ct]) with a plaintext, for `count` ciphertexts of nl limbs.  mode 0 is the CKKS multiply + relinearise of the split sequences: target / addend are the
// factors a / b, both [2][nl][N] per ciphertext.
struct KsOperands {
  int mode = 1;  // 0 multiply, 1 key switch (dispatch_mode)
  // target: the polynomial to switch, [nl][N] at target + ct * target_stride, in the ciphertext's own form (BFV coefficient, CKKS NTT);
  // addend: (c0, c1) -- c0 alone unless add_c1 -- at addend + ct * addend_stride, added to the result, or null
  const u64 *target = nullptr, *addend = nullptr;
  size_t target_stride = 0, addend_stride = 0;
  bool add_c1 = false;
  const u64 *key = nullptr;  // the key-switching key
  u64 *out = nullptr;        // [count][2][nl][N]
  const u64 *acc = nullptr;  // with gelt only: a second, ungathered ciphertext [count][2][nl][N] added in the last kernel (RotTailRoute::fused)
  // with gelt only: a CKKS plaintext, [nl][N] at plain + ct * plain_stride (0: one for all), that multiplies either component of the
  // result before acc -- which may then be null -- is added (RotTailRoute::fused)
  const u64 *plain = nullptr;
  size_t plain_stride = 0;
  u32 gelt = 0;              // the Galois element of a rotation folded into the sequence (RotRoute::fold): target = c1, addend = c0
  u32 gather = 0;            // what the kernels gather with: gelt (CKKS, NTT form) or gelt^-1 mod 2N (BFV); launch_keyswitch fills it
  int nl = 0;
  size_t count = 0;
  // the record of ciphertexts off .. off + cc - 1: the one place a chunk's pointers are computed
  KsOperands slice(size_t off, size_t cc, size_t N) const {
    const size_t ctw = 2 * (size_t)nl * N;
    KsOperands s = *this;
    s.target = target + off * target_stride;
    if (addend) s.addend = addend + off * addend_stride;
    s.out = out + off * ctw;
    if (acc) s.acc = acc + off * ctw;
    if (plain) s.plain = plain + off * plain_stride;
    s.count = cc;
    return s;
  }
};
// what the last hop of a rotation does with the rotated ciphertext r: out = r (nothing set), addend + r, or addend + plain (.) r (addend optional)
struct RotTail {
  const u64 *addend = nullptr, *plain = nullptr;
  size_t plain_stride = 0;
};

// ---- abc_buffers.hip: every allocation a recorded circuit may read, and the bodies of the C entry points of that name ----
int buffer_malloc(abc_hip_ctx *c, void **d_ptr, size_t bytes);
int buffer_free(abc_hip_ctx *c, void *d_ptr);
int trim_cache(abc_hip_ctx *c);
size_t cached_bytes(abc_hip_ctx *c);
int graph_begin(abc_hip_ctx *c);
int graph_end(abc_hip_ctx *c, void **out);
int graph_destroy(abc_hip_ctx *c, void *exec);
int held_buffers(const abc_hip_ctx *c);  // context buffers retired while a live graph owns them
void free_buffers(abc_hip_ctx *c);       // abc_hip_ctx_destroy: everything the table still tracks
// workspace / arena `which`: grow on demand (never inside a timed region after warm-up, never inside a capture)
int ensure_workspace(abc_hip_ctx *c, size_t bytes);
int ensure_aux(abc_hip_ctx *c, int which, size_t bytes);
// ABC_HIP_POISON=1: 0xFF over the workspace and every arena on c->stream (nothing while a capture is open); OpDepth calls it when
// an outermost C-ABI operation begins
void poison_arenas(abc_hip_ctx *c);
// hipMalloc of a context buffer (a key, a mirror, an arena), entered into the table; retry: flush the cache once on failure
hipError_t alloc_context_buffer(abc_hip_ctx *c, void **p, size_t bytes, bool retry);
// free context buffer p, or hold it back while a live graph owns it; the caller has drained c->stream
void retire_buffer(abc_hip_ctx *c, void *p);
void read_switches(abc_hip_ctx *c);  // the environment into c->sw, then c->facts

// ---- launchers implemented in the kernel translation units ----
LimbMap key_limb_map(const abc_hip_ctx *c, int nl);  // 0..nl-1 -> data primes, nl -> special prime
// in-place forward / inverse NTT over `limbs` consecutive limbs laid out [groups][nl][N]; limb j of each
// group uses modulus map.id[j % nl]
int launch_ntt_fwd(abc_hip_ctx *c, u64 *d, const LimbMap &map, int nl, size_t total_limbs);
int launch_ks_expand_ntt_fp(abc_hip_ctx *c, const u64 *tcoef, size_t tstride, u64 *dec, const LimbMap &map, int nl, size_t count);  // KsFront::fp
int launch_ntt_fwd_from2(abc_hip_ctx *c, const u64 *src, const u64 *src2, u64 *d, const LimbMap &map, int nl, size_t total_limbs);
int launch_ntt_fwd_from(abc_hip_ctx *c, const u64 *src, u64 *d, const LimbMap &map, int nl, size_t total_limbs);  // out of place
int launch_ntt_inv(abc_hip_ctx *c, u64 *d, const LimbMap &map, int nl, size_t total_limbs);
int launch_ntt_inv_strided_part(abc_hip_ctx *c, u64 *d, const LimbMap &map, int nl, size_t total_limbs, bool integer_only = false);
int big_block_log(void);

int launch_addsub(abc_hip_ctx *c, const u64 *a, const u64 *b, u64 *out, int nl, size_t polys, int op);  // 0 add 1 sub 2 neg
int launch_ckks_tensor(abc_hip_ctx *c, const u64 *a, const u64 *b, u64 *out3, int nl, size_t count);
// out3 [count][3][nl][N] = sum over k < n_terms of a[k] (x) b[k] (CKKS; a, b: HOST arrays of device pointers, read during the call):
// k_ckks_tensor_sum, kTensorSumTerms pointer pairs per launch by value in the kernel arguments; n_terms >= 1
constexpr int kTensorSumTerms = 8;
int launch_ckks_tensor_sum(abc_hip_ctx *c, const u64 *const *a, const u64 *const *b, int n_terms, u64 *out3, int nl, size_t count);
// out [count][size][nl][N] = (addend or 0) + sum over k < n_terms of plain[k] (.) ct[k] (CKKS; ct, plain: HOST arrays of device
// pointers, read during the call; plain_stride as ckks_multiply_plain takes it; out may be addend): k_ckks_plain_mac_sum,
// kPlainMacTerms pointer pairs per launch by value in the kernel arguments; n_terms >= 1
constexpr int kPlainMacTerms = kTensorSumTerms;
int launch_ckks_plain_mac_sum(abc_hip_ctx *c, const u64 *const *ct, const u64 *const *plain, size_t plain_stride, int n_terms, const u64 *addend,
                              u64 *out, int size, int nl, size_t count);
// out [count][size][nl][N] = (addend or 0) + cst (component 0) + sum over k < n_terms of w[k] * ct[k] (CKKS; ct: HOST array of device
// pointers, term k [count][size][ct_nl[k]][N], ct_nl[k] >= nl, its first nl limbs read in place; ct_nl null: every term at nl; w: HOST
// [n_terms][nl] canonical words, cst: HOST [nl] or null; out may be addend): k_ckks_const_mac_sum, kConstMacTerms pointers and their
// weights per launch by value in the kernel arguments; n_terms >= 0
constexpr int kConstMacTerms = kPlainMacTerms;
int launch_ckks_const_mac_sum(abc_hip_ctx *c, const u64 *const *ct, const int *ct_nl, const u64 *w, int n_terms, const u64 *cst, const u64 *addend,
                              u64 *out, int size, int nl, size_t count);
// the same sum with the rescale behind it, formed in the loads of the two LDS-resident rescale kernels (k_constsum_rescale_*): r a
// route_rescale that is not generic, every term at nl limbs, 1 <= n_terms <= kConstSumRescaleTerms
int launch_const_sum_rescale(abc_hip_ctx *c, const RescaleRoute &r, const u64 *const *ct, const u64 *w, int n_terms, const u64 *cst, const u64 *addend,
                             u64 *out, int size, int nl, size_t count);
int launch_const_plain_fill(abc_hip_ctx *c, const u64 *w, u64 *plain, int nl);  // plain [nl][N]: every word of limb j = w[j] (HOST words)
int launch_drop_to(abc_hip_ctx *c, const u64 *in, u64 *out, int from_nl, int nl, size_t polys);  // the first nl of from_nl limbs per polynomial
int keyswitch_generic(abc_hip_ctx *c, KsFront front, const KsOperands &o);
int launch_ks_tmod(abc_hip_ctx *c, const u64 *prodS, u64 *tmod, int nl, size_t polys);
int launch_ks_finish(abc_hip_ctx *c, const u64 *prodD, const u64 *tmod, u64 *out, const u64 *addend, size_t addend_stride,
                     bool add_c1, int nl, size_t count);
int launch_galois(abc_hip_ctx *c, const u64 *in, u64 *out, int nl, size_t polys, uint32_t elt, bool ntt_form);
int launch_rescale(abc_hip_ctx *c, const u64 *in, u64 *out, int size, int nl, size_t count);
int launch_mulplain_rescale(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl, size_t count);
// out [count][size][nl-1][N] = rescale((carry or 0) + sum over k < n_terms of plain[k] (.) ct[k]): the K-term forms of the LDS-resident
// rescale kernels (k_plainsum_rescale_*); r: a route_rescale that is not generic, n_terms <= kPlainMacTerms, a carry where n_terms is 0
int launch_plain_sum_rescale(abc_hip_ctx *c, const RescaleRoute &r, const u64 *const *ct, const u64 *const *plain, size_t plain_stride, int n_terms,
                             const u64 *carry, u64 *out, int size, int nl, size_t count);
int launch_drop_last(abc_hip_ctx *c, const u64 *in, u64 *out, int size, int nl, size_t count);

int bfv_multiply(abc_hip_ctx *c, BfvMul m, const u64 *a, const u64 *b, u64 *out3, size_t count);
int bfv_multiply_plain(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, size_t count);
// the NTT-domain plaintext-weighted sum (abc_kernels_bfv.hip): plain [rows][N] mod t -> [rows][L][N] lifted and transformed;
// (addend or 0) + sum_k plain_ntt[k] * ct[k] with one inverse transform, ct / plain_ntt HOST arrays of device pointers
int bfv_plain_to_ntt(abc_hip_ctx *c, const u64 *plain, u64 *plain_ntt, size_t rows);
int bfv_multiply_plain_sum(abc_hip_ctx *c, const u64 *const *ct, bool ct_ntt, const u64 *const *plain_ntt, size_t plain_stride, int n_terms,
                           const u64 *addend, u64 *out, int size, size_t count);
int bfv_addsub_plain(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, size_t count, int sub);
int ckks_multiply_plain(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl, size_t count);
int ckks_add_plain(abc_hip_ctx *c, const u64 *ct, const u64 *plain, size_t plain_stride, u64 *out, int size, int nl, size_t count, int sub);
int batch_encode(abc_hip_ctx *c, const int64_t *values, u64 *plain, size_t count);
int batch_decode(abc_hip_ctx *c, const u64 *plain, int64_t *values, size_t count);
int ckks_encode(abc_hip_ctx *c, const double *re, const double *im, size_t values_per_row, double scale, int nl, u64 *plain,
                size_t count);  // abc_kernels_ckks_codec.hip
int ckks_decode(abc_hip_ctx *c, const u64 *plain, int nl, double scale, double *re, double *im, size_t count);
int encrypt(abc_hip_ctx *c, const u64 *plain, uint64_t seed, u64 *ct, size_t count);
int decrypt(abc_hip_ctx *c, const u64 *ct, int size, int nl, u64 *plain, size_t count);
int noise_budget(abc_hip_ctx *c, const u64 *ct, int size, int nl, int *h_budget, size_t count);  // abc_keys.hip
int keygen(abc_hip_ctx *c, uint64_t seed);
int keygen_secure(abc_hip_ctx *c);
int encrypt_secure(abc_hip_ctx *c, const u64 *plain, u64 *ct, size_t count);
int microbench(abc_hip_ctx *c, int which, int iters, double *ms);
// ---- the keyed sampling spec (abc_sample.hpp): kernels in abc_kernels_sample.hip, entry points in abc_keys.hip ----
constexpr size_t kSampleKeyBytes = 64;  // device key buffer: 8 key words, the 64-bit nonce, padding
int upload_sample_key(abc_hip_ctx *c, void *d_kb, const uint8_t key[32], uint64_t nonce);
int launch_sample_small(abc_hip_ctx *c, const void *d_kb, uint64_t stream_off, size_t streams, size_t polys, size_t ternaries,
                        int8_t *d_out);
int launch_sample_uniform(abc_hip_ctx *c, const void *d_kb, uint64_t stream_off, int nkeys, u64 *d_a);
int encrypt_keyed(abc_hip_ctx *c, const u64 *plain, const uint8_t key[32], uint64_t nonce, u64 *ct, size_t count);
int keygen_keyed(abc_hip_ctx *c, const uint8_t key_sec[32], const uint8_t key_pub[32]);
int keyed_small(abc_hip_ctx *c, const uint8_t key[32], uint64_t nonce, int8_t *d_small, size_t count);
int keyed_uniform(abc_hip_ctx *c, const uint8_t key[32], uint64_t stream, int nkeys, u64 *d_a);

// the key switch o along route r (abc_kernels_fused.hip; any sequence).  o.gelt, o.acc and o.plain are checked here, once, against what the
// sequence can do (seq_folds_permutation, seq_takes_acc, seq_takes_plain); the sequences below check nothing again
int launch_keyswitch(abc_hip_ctx *c, const KsRoute &r, const KsOperands &o);
// CKKS multiply + relinearise in one sequence (every Seq but bmul and generic)
int launch_mul_relin(abc_hip_ctx *c, Seq seq, const u64 *a, const u64 *b, u64 *out, int nl, size_t count);
// split key switch without LDS-resident limbs (abc_kernels_gsplit.hip): N = 2^15, and the first step at N = 2^14 for small batches
size_t gsplit_scratch_words(const abc_hip_ctx *c, int nl);
int gsplit_chunk15(abc_hip_ctx *c, hipStream_t st, u64 *scratch, const KsOperands &o);  // o: one chunk
void gsplit_front14(hipStream_t st, abc_hip_ctx *c, const KsOperands &o, double *hinv, double *part, int pack);
// ---- the main step of the split key switch (k_split4_main_fp, k_gsplit_main[_deep], k_isplit_main[_deep]): host side ----
// its arguments, as the launchers pass them along (the kernels' own argument lists are spelled once, at the launch)
constexpr u64 kAllSlots = 0xfedcba9876543210ull;
struct MainArgs {
  hipStream_t st = nullptr;
  KsOperands ops;                                // the chunk
  const void *part = nullptr, *tpart = nullptr;  // half-done decomposition / mod-down limbs (doubles or u64: the arithmetic of the kernel)
  u64 imap = kAllSlots;  // nibble s = data prime of grid slot s (kAllSlots with ni = nl: all of them; the 512-thread kernels read eight nibbles)
  int ni = 0;            // slots
  int pack = 0;          // the half-done limbs are packed (abc_ntt.hpp; k_split4_main_fp only)
};
// The last kernels of the split key switches take the tail of a rotation (RotTail, as o.acc / o.plain / o.plain_stride) as a
// trailing template parameter PACK: empty without a tail (the name, argument list and code the kernel had before there were
// tails), <.., WithAcc> with one more argument, the pointer, for the second addend of rotate_add, <.., WithMac> below.  The host
// launches each of them once, from dispatch_tail: `tag` names the pack an argument belongs to.
struct WithAcc {};
template <class T>
struct AccArg {
  using tag = T;
  const u64 *p;
};
__host__ __device__ inline const u64 *acc_ptr() { return nullptr; }
__host__ __device__ inline const u64 *acc_ptr(AccArg<WithAcc> a) { return a.p; }
// <.., WithMac>: rotate_mac_plain, out = acc + plain (.) result.  One more argument again, the three operands: the plaintext
// [nl][N] at plain + ct * plain_stride, read like acc at the thread's own index, and acc itself, null where there is none
// (a workgroup-uniform branch).  The finished pair is multiplied and added in registers ahead of its only store.
struct WithMac {};
template <>
struct AccArg<WithMac> {
  using tag = WithMac;
  const u64 *plain;
  size_t plain_stride;
  const u64 *p;
};
__host__ __device__ inline const u64 *acc_ptr(AccArg<WithMac> a) { return a.p; }
__host__ __device__ inline AccArg<WithMac> mac_arg() { return {nullptr, 0, nullptr}; }
template <class T>
__host__ __device__ inline AccArg<WithMac> mac_arg(AccArg<T>) { return {nullptr, 0, nullptr}; }
__host__ __device__ inline AccArg<WithMac> mac_arg(AccArg<WithMac> a) { return a; }
template <class... A>
inline constexpr bool kWithAcc = (std::is_same_v<A, WithAcc> || ...);
template <class... A>
inline constexpr bool kWithMac = (std::is_same_v<A, WithMac> || ...);
// nl + 1 transform buffers + the block's twiddle table, 1024 entries of tw_bytes = sizeof(A::TW): 8 (fp64) or 16 (integer)
constexpr size_t main_lds_bytes(int nl, int tw_bytes) { return (size_t)((nl + 1) * lds_words(10)) * 8 + 1024 * (size_t)tw_bytes; }
// (o.mode, o.gather) -> f(MODE, GAL) as integral constants: multiply / key switch with the Galois gather folded in / plain key switch
template <class Fn>
inline void dispatch_mode(int mode, u32 gelt, Fn f) {
  if (mode == 0) f(std::integral_constant<int, 0>{}, std::false_type{});
  else if (gelt) f(std::integral_constant<int, 1>{}, std::true_type{});
  else f(std::integral_constant<int, 1>{}, std::false_type{});
}
// the trailing operands of o as the pack its last kernel is instantiated with: f(), f(AccArg<WithAcc>) or f(AccArg<WithMac>).
// ACC_OK / MAC_OK: the launch site has that form of its kernel (launch_keyswitch has checked o against the sequence: the forms
// a site lacks do not reach it); f is instantiated for those alone
template <bool ACC_OK, bool MAC_OK, class Fn>
inline void dispatch_tail(const KsOperands &o, Fn f) {
  if constexpr (MAC_OK) {
    if (o.plain) return f(AccArg<WithMac>{o.plain, o.plain_stride, o.acc});
  }
  if constexpr (ACC_OK) {
    if (o.acc) return f(AccArg<WithAcc>{o.acc});
  }
  f();
}
// logn -> f(LB) as an integral constant and its result; a ring outside [LO, HI] is an error (the routes keep it from happening)
template <int LO, int HI, class Fn>
inline int dispatch_logn(int logn, Fn f) {
  if constexpr (LO <= HI) {
    if (logn == LO) return f(std::integral_constant<int, LO>{});
    return dispatch_logn<LO + 1, HI>(logn, f);
  } else {
    set_error("no kernel of this sequence for the ring degree");
    return 1;
  }
}
// nl -> f(NL) as an integral constant, NL = nl clamped to [LO, HI]
template <int LO, class Fn, int... Is>
inline void dispatch_nl_seq(int nl, Fn &f, std::integer_sequence<int, Is...>) {
  (void)(((nl == LO + Is) && (f(std::integral_constant<int, LO + Is>{}), true)) || ...);
}
template <int LO, int HI, class Fn>
inline void dispatch_nl(int nl, Fn f) {
  dispatch_nl_seq<LO>(nl < LO ? LO : nl > HI ? HI : nl, f, std::make_integer_sequence<int, HI - LO + 1>{});
}
// over the slots of a.imap: all data primes, or the fp64-capable ones of a mixed chain (abc_kernels_isplit.hip).
// split4_main (N = 2^14): false = not applicable (more than seven limbs); gsplit_main15: any nl <= 15 (above seven: the deep kernel)
bool split4_main(abc_hip_ctx *c, const MainArgs &a);
void gsplit_main15(abc_hip_ctx *c, const MainArgs &a);
int bsplit_big(abc_hip_ctx *c, const KsOperands &o);
// BFV, N = 2^LOGN (13, 14): the steps behind a `part` already written, on one chunk; reads o's key, addend, out, gather, acc
// (N = 2^14 only)
template <int LOGN>
int bsplit_back(abc_hip_ctx *c, hipStream_t st, const double *part, double *half, const KsOperands &o);
// the mirrors of a key-switching key (nullptr: not available -- capture in progress and not built yet, or allocation failed)
const double *key_twin(abc_hip_ctx *c, const u64 *key);
const double *key_twin_lookup(const abc_hip_ctx *c, const u64 *key);  // never builds: safe once the lanes have forked
const u64 *key_shoup(abc_hip_ctx *c, const u64 *key);
// key'_g of a hoisted rotation: `key` with every [N] row permuted by ginv = g^-1 mod 2N in NTT form.  Built on
// c->stream on first use, whatever ABC_HIP_NO_KEY_TWIN says (it is semantics, not an optimisation); nullptr with the error set:
// allocation failed, or a capture is in progress and it is not built yet
const u64 *key_permuted(abc_hip_ctx *c, const u64 *key, u32 ginv);
// rewrite the existing mirrors of `key` (nullptr: of every key) from its current words, in the same buffers, on c->stream: a
// recorded circuit keeps their addresses and reads the new key
int refresh_key_mirrors(abc_hip_ctx *c, const u64 *key /* nullptr: all */);  // non-zero: a launch failed, error set
// a key-switching key that goes (keygen drops a non-default Galois element): the key and its mirrors are retired
void release_key(abc_hip_ctx *c, u64 *key);
// internal lanes (streams forked off the context's stream): chunks of one call alternate over them (abc_kernels_fused.hip)
int fork_lanes(abc_hip_ctx *c, int lanes);
int join_lanes(abc_hip_ctx *c, int lanes);
// fork on construction (fork()), join on every way out: an early `return 1` between the two would otherwise leave work on
// the lanes that the context's stream -- and with it every later use or release of the buffers involved -- never waits for
struct LaneScope {
  abc_hip_ctx *c;
  int lanes;
  bool forked = false;
  LaneScope(abc_hip_ctx *c_, int lanes_) : c(c_), lanes(lanes_) {}
  int fork() {
    if (fork_lanes(c, lanes)) return 1;
    forked = true;
    return 0;
  }
  int join() {
    forked = false;
    return join_lanes(c, lanes);
  }
  ~LaneScope() {
    if (forked) (void)join_lanes(c, lanes);
  }
};

// One call's chunk / lane loop: `count` ciphertexts in chunks of `chunk`, chunk `turn` on lane `turn % lanes` (fewer than two
// lanes: the context's stream) with that lane's scratch, `per_ct` words per ciphertext, lane l's starting at l * chunk * per_ct.
// The workspace grows and the fp64 twin of `twin_key` (nullptr: none needed) is built BEFORE the lanes fork: a capture must not
// allocate after them.  body(stream, scratch, off, cc) enqueues ciphertexts off .. off + cc - 1 and returns non-zero on error.
template <class Body>
int for_each_chunk(abc_hip_ctx *c, size_t count, size_t chunk, int lanes, size_t per_ct, const u64 *twin_key, Body body) {
  if (ensure_workspace(c, (size_t)lanes * chunk * per_ct * 8)) return 1;
  if (twin_key) (void)key_twin(c, twin_key);
  LaneScope scope(c, lanes);
  if (scope.fork()) return 1;
  int turn = 0;
  for (size_t off = 0; off < count; off += chunk, turn++) {
    const size_t cc = (count - off < chunk) ? count - off : chunk;
    const int l = (lanes > 1) ? turn % lanes : 0;
    if (body((lanes > 1) ? c->lane[l] : c->stream, (u64 *)c->ws + (size_t)l * chunk * per_ct, off, cc)) return 1;
  }
  return scope.join();
}
// single-stream calls: as many ciphertexts per chunk as `budget_bytes` of scratch hold (at least 1, at most count), in even
// chunks without a runt when there are fewer than 8 of them
inline size_t even_chunks(size_t budget_bytes, size_t per_ct_words, size_t count) {
  size_t chunk = budget_bytes / 8 / per_ct_words;
  if (chunk < 1) chunk = 1;
  if (chunk > count) chunk = count;
  else if (count % chunk && count / chunk < 8) chunk = (count + count / chunk) / (count / chunk + 1);
  return chunk;
}

// Prime-width predicates for the per-launch arithmetic choices (launch_ntt, the BFV tensor kernels, multiply_plain); which
// SEQUENCE runs is abc_route.hpp's business.  The name says WHICH primes are inspected, `ok` is the width test.
template <class P>
inline bool all_data_primes(const abc_hip_ctx *c, int nl, P ok) {  // the first nl data primes, not the special prime
  for (int j = 0; j < nl; j++)
    if (!ok(c->h_mods[j].bits)) return false;
  return true;
}
template <class P>
inline bool all_mapped_primes(const abc_hip_ctx *c, const LimbMap &map, int nl, P ok) {  // the moduli map.id[0 .. nl-1]
  for (int j = 0; j < nl; j++)
    if (!ok(c->h_mods[map.id[j]].bits)) return false;
  return true;
}

// BFV multiply (+ relinearise) in split form, N = 2^14 (abc_kernels_bmul.hip)
int bmul_split(abc_hip_ctx *c, const u64 *a, const u64 *b, u64 *out, size_t count, bool relin);  // Seq::bmul / BfvMul::split
int bmul_big(abc_hip_ctx *c, const u64 *a, const u64 *b, u64 *out3, size_t count);                 // BfvMul::big
// integer twins of the split kernels (abc_kernels_isplit.hip)
size_t isplit_scratch_words(const abc_hip_ctx *c, int nl);
int isplit_chunk(abc_hip_ctx *c, hipStream_t st, u64 *scratch, const KsOperands &o, const ChunkRoute &k);  // o: one chunk

}  // namespace abc
