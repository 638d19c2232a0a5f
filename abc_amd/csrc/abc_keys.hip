// abc_keys.hip -- key generation, encryption and decryption on the device.
//
// Reference call sites replaced (src/runtime/SealCiphertextFactory.cpp):
//   :89-93  seal::KeyGenerator: secret_key(), create_public_key, create_galois_keys (all default
//           elements), create_relin_keys                                       -> keygen
//   :12     seal::Encryptor::encrypt (public key, then modulus switch to the data level) -> encrypt
//   :150    seal::Decryptor::decrypt                                           -> decrypt
// and src/runtime/SealCiphertext.cpp:80-83 seal::Decryptor::invariant_noise_budget -> noise_budget
// Randomness follows this repo's two sampling specs (SEAL's own PRNG stream is not reproducible by
// design).  The seeded spec (Rng below: splitmix64-seeded xoshiro256**, ternary secrets, 21-vs-21-bit centred binomial errors,
// rejection sampled uniform residues) is sequential: it is drawn on the host and only the small polynomials travel to the
// device.  The keyed spec (abc_sample.hpp: counter-based ChaCha20, no rejection, the library's only cipher) is drawn on the
// device by abc_kernels_sample.hip, or word for word by its host twin under ABC_HIP_HOST_SAMPLING=1; it serves the keyed entry
// points, and the OS-keyed ones are the keyed ones under keys from getrandom(2).  All ring arithmetic (NTTs, products, modulus
// switching) runs in HIP kernels either way.
#include <algorithm>
#include <cstring>
#include <sys/random.h>
#include <thread>
#include <vector>

#include "abc_context.hpp"
#include "abc_crt_lift.hpp"
#include "abc_host_math.hpp"
#include "abc_sample.hpp"

namespace abc {

int launch_bfv_decrypt_round(abc_hip_ctx *c, const u64 *phase, u64 *plain, size_t count);

// ---------------- host samplers ----------------
// Rng (splitmix64-seeded xoshiro256**) is this repo's SAMPLING SPEC for parity tests: the oracle implements the same stream, so
// keys and ciphertexts are bit-comparable -- it is NOT a cryptographic generator (64-bit seed, linear state) and is only reached
// through the explicitly seeded entry points.  A plain struct: every draw inlines into its loop.  Everything else (the keyed and
// the OS-keyed entry points) draws the keyed spec of abc_sample.hpp, whose host twin needs no generator state.
struct Rng {
  uint64_t s[4];
  explicit Rng(uint64_t seed) {
    uint64_t x = seed;
    for (auto &w : s) {
      uint64_t z = (x += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      w = z ^ (z >> 31);
    }
  }
  static uint64_t rotl(uint64_t v, int k) { return (v << k) | (v >> (64 - k)); }
  uint64_t next() {
    const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl(s[3], 45);
    return r;
  }
  int8_t ternary() {
    for (;;) {
      const uint64_t x = next();
      if (x != ~0ull) return (int8_t)((int)(x % 3) - 1);
    }
  }
  int8_t cbd() {
    const uint64_t x = next();
    return (int8_t)(__builtin_popcountll(x & 0x1FFFFF) - __builtin_popcountll((x >> 21) & 0x1FFFFF));
  }
  // uniform residue modulo q by rejection; lim = reject_limit(q), which a caller computes once per prime, not once per draw
  static uint64_t reject_limit(uint64_t q) { return ~0ull - (~0ull % q) - 1; }
  uint64_t uniform(uint64_t q, uint64_t lim) {
    uint64_t x;
    do x = next(); while (x >= lim);
    return x % q;
  }
};

static int getrandom_fill(uint8_t *p, size_t bytes) {
  size_t got = 0;
  while (got < bytes) {
    const ssize_t r = getrandom(p + got, bytes - got, 0);
    if (r <= 0) return 1;
    got += (size_t)r;
  }
  return 0;
}
// host draws to the device; the host copy is wiped once the upload has completed
static int upload_wiped(abc_hip_ctx *c, void *dst, void *h, size_t bytes) {
  const hipError_t e = hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, c->stream);
  const hipError_t s = hipStreamSynchronize(c->stream);  // h is the caller's local
  explicit_bzero(h, bytes);
  ABC_HIP_CHECK(e);
  ABC_HIP_CHECK(s);
  return 0;
}

// ---------------- kernels ----------------
// small signed polynomial [polys][N] (int8) -> residues [polys][nlm][N] for the mapped moduli
// polynomial p sits at small[(p / per) * group_stride + offset + (p % per) * N]
__global__ __launch_bounds__(256) void k_small_to_rns(DevCtx c, const int8_t *small, size_t per, size_t group_stride, size_t offset,
                                                      u64 *out, LimbMap map, int nlm, size_t polys) {
  const size_t items = polys * nlm * (size_t)c.n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t limb = it >> c.logn, x = it & (c.n - 1);
    const size_t p = limb / nlm;
    const u64 q = c.mods[map.id[limb % nlm]].q;
    const int v = small[(p / per) * group_stride + offset + (p % per) * c.n + x];
    out[it] = v < 0 ? q - (u64)(-v) : (u64)v;
  }
}

// out[polys][nlm][N] = a * b (b broadcast with stride b_stride words per poly)
__global__ __launch_bounds__(256) void k_dyadic_mul(DevCtx c, const u64 *a, const u64 *b, size_t b_stride, u64 *out, LimbMap map,
                                                    int nlm, size_t polys) {
  const size_t pw = (size_t)nlm * c.n;
  const size_t items = polys * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t p = it / pw, w = it % pw;
    out[it] = mul_mod(a[it], b[p * b_stride + w], c.mods[map.id[w >> c.logn]]);
  }
}

// acc[polys][nlm][N] += x   (x per-poly stride x_stride)
__global__ __launch_bounds__(256) void k_acc_add(DevCtx c, u64 *acc, const u64 *x, size_t x_stride, LimbMap map, int nlm,
                                                 size_t polys) {
  const size_t pw = (size_t)nlm * c.n;
  const size_t items = polys * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t p = it / pw, w = it % pw;
    acc[it] = add_mod(acc[it], x[p * x_stride + w], c.mods[map.id[w >> c.logn]].q);
  }
}

// key-switch key assembly (KeyGenerator::generate_one_kswitch_key):
//   key[i][0][j] = -(a_i[j]*s[j] + e_i[j]) (+ (q_sp mod q_i) * new_key[i] when j == i),  key[i][1][j] = a_i[j]
// a: [L][K][N] uniform (NTT domain), e: [L][K][N] error already in NTT form, s/new_key: [K][N] NTT form
__global__ __launch_bounds__(256) void k_make_kskey(DevCtx c, const u64 *a, const u64 *e, const u64 *s, const u64 *new_key,
                                                    u64 *key, int nkeys) {
  const size_t pw = (size_t)c.K * c.n;
  const size_t items = (size_t)nkeys * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int i = (int)(it / pw);
    const size_t w = it % pw;
    const int j = (int)(w >> c.logn);
    const size_t x = w & (c.n - 1);
    const Mod m = c.mods[j];
    const u64 av = a[it];
    u64 v = neg_mod(add_mod(mul_mod(av, s[w], m), e[it], m.q), m.q);
    if (new_key && j == i) v = add_mod(v, mul_mod(new_key[(size_t)i * c.n + x], c.cst->special_mod_q[i], m), m.q);
    key[((size_t)i * 2 + 0) * pw + w] = v;
    key[((size_t)i * 2 + 1) * pw + w] = av;
  }
}

// prodS/prodD split of [polys][K][N] into data limbs [polys][L][N] and the special limb [polys][N]
static int split_special(abc_hip_ctx *c, const u64 *full, u64 *data, u64 *special, size_t polys) {
  const size_t N = (size_t)c->n;
  ABC_HIP_CHECK(hipMemcpy2DAsync(data, c->L * N * 8, full, c->K * N * 8, c->L * N * 8, polys, hipMemcpyDeviceToDevice, c->stream));
  ABC_HIP_CHECK(hipMemcpy2DAsync(special, N * 8, full + (size_t)c->L * N, c->K * N * 8, N * 8, polys, hipMemcpyDeviceToDevice,
                                 c->stream));
  return 0;
}

// c[ct][p][j] = u[ct][j] * pk[p][j]   (key level, NTT form)
__global__ __launch_bounds__(256) void k_enc_mul_pk(DevCtx c, const u64 *u, const u64 *pk, u64 *cfull, size_t count) {
  const size_t pw = (size_t)c.K * c.n;
  const size_t items = count * 2 * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ct = it / (2 * pw), r = it % (2 * pw);
    const size_t w = r % pw;
    cfull[it] = mul_mod(u[ct * pw + w], pk[r], c.mods[w >> c.logn]);
  }
}

// ---------------- key generation ----------------
// Where the draws of a key set come from: one policy per sampling path (seeded host, keyed host, keyed device), all with the
// same four members.
//   begin(c, d_kb)   once the staging buffers exist; d_kb: 2 * kSampleKeyBytes of device memory behind the int8 staging
//   secret(c, d_e8)  the ternary secret key, N int8 on the device
//   key(c, stream, nkeys, d_a, d_e8)  the uniform a [nkeys][K][N] (published) and the errors [nkeys][N] (secret) of one key
//   staged(c)        after the kernels that read d_a / d_e8 are enqueued (a host policy waits: its staging is reused)
// The two host policies are HostDraws over a Fill: the staging, the uploads and the wipes are one body, and a Fill (plain data:
// it is wiped byte-wise) only says how the words come about -- secret(c, e) and key(c, stream, nkeys, a, e) into host memory.
template <class Fill>
struct HostDraws {
  Fill fill;
  std::vector<uint64_t> h_a;
  std::vector<int8_t> h_e;
  template <class... A>
  explicit HostDraws(A &&...a) : fill(a...) {}  // in place: no second copy of a key to wipe
  ~HostDraws() {
    explicit_bzero(&fill, sizeof(fill));  // generator state or sampling keys
    if (!h_e.empty()) explicit_bzero(h_e.data(), h_e.size());
  }
  int begin(abc_hip_ctx *c, void *) {
    h_a.resize((size_t)c->L * c->K * c->n);
    h_e.resize((size_t)c->L * c->n);
    return 0;
  }
  int secret(abc_hip_ctx *c, int8_t *d_e8) {
    fill.secret(c, h_e.data());
    ABC_HIP_CHECK(hipMemcpyAsync(d_e8, h_e.data(), (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    return 0;
  }
  int key(abc_hip_ctx *c, uint64_t stream, int nkeys, u64 *d_a, int8_t *d_e8) {
    const size_t N = (size_t)c->n;
    fill.key(c, stream, nkeys, h_a.data(), h_e.data());
    ABC_HIP_CHECK(hipMemcpyAsync(d_a, h_a.data(), (size_t)nkeys * c->K * N * 8, hipMemcpyHostToDevice, c->stream));
    ABC_HIP_CHECK(hipMemcpyAsync(d_e8, h_e.data(), (size_t)nkeys * N, hipMemcpyHostToDevice, c->stream));
    return 0;
  }
  int staged(abc_hip_ctx *c) {
    ABC_HIP_CHECK(hipStreamSynchronize(c->stream));  // host staging buffers are reused by the next key
    return 0;
  }
};
// the seeded spec: one sequential stream, in the order secret key, then per key a_i (limb by limb), e_i
struct SeededFill {
  Rng rng;
  explicit SeededFill(uint64_t seed) : rng(seed) {}
  void secret(const abc_hip_ctx *c, int8_t *e) {
    for (size_t x = 0; x < (size_t)c->n; x++) e[x] = rng.ternary();
  }
  void key(const abc_hip_ctx *c, uint64_t, int nkeys, uint64_t *a, int8_t *e) {
    const size_t N = (size_t)c->n;
    const int K = c->K;
    for (int i = 0; i < nkeys; i++) {
      for (int j = 0; j < K; j++) {  // 156 M draws for a key set at N = 2^16: the rejection limit once per prime
        const uint64_t q = c->primes[j], lim = Rng::reject_limit(q);
        uint64_t *row = a + ((size_t)i * K + j) * N;
        for (size_t x = 0; x < N; x++) row[x] = rng.uniform(q, lim);
      }
      for (size_t x = 0; x < N; x++) e[(size_t)i * N + x] = rng.cbd();
    }
  }
};
// host twin of launch_sample_uniform: a [nkeys][K][N] of (key words, stream)
static void sample_uniform_host(const abc_hip_ctx *c, const uint32_t k[8], uint64_t stream, int nkeys, uint64_t *a) {
  keyed::uniform_host(k, stream, (size_t)c->n, c->K, c->primes.data(), nkeys, a);
}
// the keyed spec on the host (ABC_HIP_HOST_SAMPLING=1): the same words as KeyedDraws from the host twin
struct KeyedHostFill {
  uint32_t sec[8], pub[8];
  KeyedHostFill(const uint8_t key_sec[32], const uint8_t key_pub[32]) {
    keyed::load_key(key_sec, sec);
    keyed::load_key(key_pub, pub);
  }
  void secret(const abc_hip_ctx *c, int8_t *e) { keyed::small_host(sec, keyed::kStreamSecret, (size_t)c->n, 1, 1, e); }
  void key(const abc_hip_ctx *c, uint64_t stream, int nkeys, uint64_t *a, int8_t *e) {
    sample_uniform_host(c, pub, stream, nkeys, a);
    keyed::small_host(sec, stream, (size_t)c->n, (size_t)nkeys, 0, e);
  }
};
// the keyed spec on the device: nothing is staged on the host, and no key costs an upload or a synchronisation
struct KeyedDraws {
  const uint8_t *key_sec, *key_pub;
  const void *d_sec = nullptr, *d_pub = nullptr;
  int begin(abc_hip_ctx *c, void *d_kb) {
    d_sec = d_kb;
    d_pub = (const char *)d_kb + kSampleKeyBytes;
    return upload_sample_key(c, (void *)d_sec, key_sec, 0) || upload_sample_key(c, (void *)d_pub, key_pub, 0);
  }
  int secret(abc_hip_ctx *c, int8_t *d_e8) { return launch_sample_small(c, d_sec, keyed::kStreamSecret, 1, 1, 1, d_e8); }
  int key(abc_hip_ctx *c, uint64_t stream, int nkeys, u64 *d_a, int8_t *d_e8) {
    return launch_sample_uniform(c, d_pub, stream, nkeys, d_a) || launch_sample_small(c, d_sec, stream, 1, (size_t)nkeys, 0, d_e8);
  }
  int staged(abc_hip_ctx *) { return 0; }
};

// The device staging of one key generation: a [L][K][N] | e in residues [L][K][N] | e as int8 [L][N], the two sampling keys of the
// keyed spec behind it | new key [K][N].  All but a hold secret material (the secret key, s^2 / g(s), the errors, the sampling
// keys): however keygen_with ends, they are zeroed on the stream before they are freed.  Reports nothing: a failure on this way
// out cannot be acted on.
struct KeygenStaging {
  abc_hip_ctx *c;
  const size_t ae_bytes, e8_bytes, newkey_bytes;
  u64 *d_a = nullptr, *d_e = nullptr, *d_newkey = nullptr;
  int8_t *d_e8 = nullptr;
  bool wiped = false;
  explicit KeygenStaging(abc_hip_ctx *ctx)
      : c(ctx), ae_bytes((size_t)c->L * c->K * c->n * 8), e8_bytes((size_t)c->L * c->n + 2 * kSampleKeyBytes),
        newkey_bytes((size_t)c->K * c->n * 8) {}
  KeygenStaging(const KeygenStaging &) = delete;
  KeygenStaging &operator=(const KeygenStaging &) = delete;
  int alloc() {
    ABC_HIP_CHECK(hipMalloc(&d_a, ae_bytes));
    ABC_HIP_CHECK(hipMalloc(&d_e, ae_bytes));
    ABC_HIP_CHECK(hipMalloc(&d_e8, e8_bytes));
    ABC_HIP_CHECK(hipMalloc(&d_newkey, newkey_bytes));
    return 0;
  }
  void *sample_keys() const { return d_e8 + (e8_bytes - 2 * kSampleKeyBytes); }
  hipError_t wipe() {
    wiped = true;
    if (d_e) (void)hipMemsetAsync(d_e, 0, ae_bytes, c->stream);
    if (d_e8) (void)hipMemsetAsync(d_e8, 0, e8_bytes, c->stream);
    if (d_newkey) (void)hipMemsetAsync(d_newkey, 0, newkey_bytes, c->stream);
    return hipStreamSynchronize(c->stream);
  }
  ~KeygenStaging() {
    if (!wiped) (void)wipe();
    (void)hipFree(d_a); (void)hipFree(d_e); (void)hipFree(d_e8); (void)hipFree(d_newkey);
  }
};

template <class D>
static int make_kskey(abc_hip_ctx *c, D &draws, uint64_t stream, const u64 *d_new_key, u64 *d_key, const KeygenStaging &st,
                      int nkeys) {
  const size_t N = (size_t)c->n;
  const int K = c->K;
  if (draws.key(c, stream, nkeys, st.d_a, st.d_e8)) return 1;
  const LimbMap kmap = key_limb_map(c, c->L);  // the identity over the K key limbs
  hipLaunchKernelGGL(k_small_to_rns, dim3(grid_for((size_t)nkeys * K * N, 256)), dim3(256), 0, c->stream, c->dc, st.d_e8, (size_t)1,
                     N, (size_t)0, st.d_e, kmap, K, (size_t)nkeys);
  ABC_HIP_CHECK(hipGetLastError());
  if (launch_ntt_fwd(c, st.d_e, kmap, K, (size_t)nkeys * K)) return 1;
  hipLaunchKernelGGL(k_make_kskey, dim3(grid_for((size_t)nkeys * K * N, 256)), dim3(256), 0, c->stream, c->dc, st.d_a, st.d_e,
                     c->d_sk, d_new_key, d_key, nkeys);
  ABC_HIP_CHECK(hipGetLastError());
  return draws.staged(c);
}

template <class D>
static int keygen_with(abc_hip_ctx *c, D &draws) {
  const size_t N = (size_t)c->n;
  const int K = c->K, L = c->L;
  const LimbMap kmap = key_limb_map(c, L);
  KeygenStaging st(c);
  if (st.alloc()) return 1;
  u64 *const d_newkey = st.d_newkey;
  if (draws.begin(c, st.sample_keys())) return 1;
  // secret key
  if (draws.secret(c, st.d_e8)) return 1;
  if (!c->d_sk) ABC_HIP_CHECK(alloc_context_buffer(c, (void **)&c->d_sk, (size_t)K * N * 8, false));
  hipLaunchKernelGGL(k_small_to_rns, dim3(grid_for((size_t)K * N, 256)), dim3(256), 0, c->stream, c->dc, st.d_e8, (size_t)1, N,
                     (size_t)0, c->d_sk, kmap, K, (size_t)1);
  ABC_HIP_CHECK(hipGetLastError());
  if (launch_ntt_fwd(c, c->d_sk, kmap, K, K)) return 1;
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  // public key = one symmetric encryption of zero at key level
  if (!c->d_pk) ABC_HIP_CHECK(alloc_context_buffer(c, (void **)&c->d_pk, (size_t)2 * K * N * 8, false));
  if (make_kskey(c, draws, keyed::kStreamPublic, nullptr, c->d_pk, st, 1)) return 1;
  // relinearisation key: switches s^2 -> s.  Every key-switching key is regenerated into the buffer it already has, and its
  // mirrors are rebuilt in place at the end: a recorded circuit keeps the addresses it baked in (include/abc_hip.h, graphs).
  if (!c->d_relin) ABC_HIP_CHECK(alloc_context_buffer(c, (void **)&c->d_relin, c->key_words() * 8, false));
  hipLaunchKernelGGL(k_dyadic_mul, dim3(grid_for((size_t)K * N, 256)), dim3(256), 0, c->stream, c->dc, c->d_sk, c->d_sk,
                     (size_t)0, d_newkey, kmap, K, (size_t)1);
  ABC_HIP_CHECK(hipGetLastError());
  if (make_kskey(c, draws, keyed::kStreamRelin, d_newkey, c->d_relin, st, L)) return 1;
  // Galois keys for the default element set (GaloisTool::get_elts_all): 2N-1, then 3^(2^i), 3^-(2^i); an element the caller had
  // loaded outside that set goes
  std::map<uint32_t, uint64_t *> old_galois;
  old_galois.swap(c->d_galois);
  c->galois_order.clear();
  const uint64_t m = 2 * (uint64_t)N;
  std::vector<uint32_t> elts;
  elts.push_back((uint32_t)(m - 1));
  uint64_t pos = 3, neg = host::invmod(3, m);
  for (int i = 0; i < c->logn - 1; i++) {
    elts.push_back((uint32_t)pos); pos = (pos * pos) & (m - 1);
    elts.push_back((uint32_t)neg); neg = (neg * neg) & (m - 1);
  }
  for (uint32_t elt : elts) {
    if (c->d_galois.count(elt)) continue;  // 3^(N/4) = 3^-(N/4) mod 2N is listed twice: first key wins
    u64 *d_key = nullptr;
    auto reuse = old_galois.find(elt);
    if (reuse != old_galois.end()) {
      d_key = reuse->second;
      old_galois.erase(reuse);
    } else {
      ABC_HIP_CHECK(alloc_context_buffer(c, (void **)&d_key, c->key_words() * 8, false));
    }
    if (launch_galois(c, c->d_sk, d_newkey, K, 1, elt, true)) return 1;
    if (make_kskey(c, draws, keyed::galois_stream(elt), d_newkey, d_key, st, L)) return 1;
    c->d_galois[elt] = d_key;
    c->galois_order.push_back(elt);
  }
  ABC_HIP_CHECK(st.wipe());  // before anything is released
  for (auto &kv : old_galois) release_key(c, kv.second);  // held back while a live graph may read it
  if (refresh_key_mirrors(c, nullptr)) return 1;
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}
int keygen(abc_hip_ctx *c, uint64_t seed) {
  HostDraws<SeededFill> draws(seed);
  return keygen_with(c, draws);
}
int keygen_keyed(abc_hip_ctx *c, const uint8_t key_sec[32], const uint8_t key_pub[32]) {
  if (!key_sec || !key_pub) { set_error("keygen_keyed: null key"); return 1; }
  if (c->sw.host_sampling) {
    HostDraws<KeyedHostFill> draws(key_sec, key_pub);
    return keygen_with(c, draws);
  }
  KeyedDraws draws{key_sec, key_pub};
  return keygen_with(c, draws);
}
int keygen_secure(abc_hip_ctx *c) {
  uint8_t keys[2][32];  // two independent keys from the operating system: [0] secret material, [1] published material
  int rc = getrandom_fill(&keys[0][0], sizeof(keys));
  if (rc) set_error("keygen: getrandom failed");
  else rc = keygen_keyed(c, keys[0], keys[1]);
  explicit_bzero(keys, sizeof(keys));
  return rc;
}

// ---------------- encryption ----------------
// workspace of one call: key 64 bytes | small [count][3][N] int8 | u [K][N] | cfull [2][K][N] | err [2][K][N] | prodD [2][L][N] |
// prodS [2][N] | tmod [2][L][N] (u and everything behind it per ciphertext).  The sampling key of the keyed spec, the draws and
// everything derived from them before the modulus switch are the first wipe_bytes.
struct EncryptWs {
  void *d_kb;
  int8_t *d_small;
  u64 *u, *cfull, *err, *prodD, *prodS, *tmod;
  size_t wipe_bytes;
};
static int encrypt_workspace(abc_hip_ctx *c, size_t count, EncryptWs &w) {
  const size_t N = (size_t)c->n;
  const size_t K = (size_t)c->K, L = (size_t)c->L;
  const size_t per_ct_words = (K + 2 * K + 2 * K + 2 * L + 2 + 2 * L) * N;
  const size_t small_bytes = (count * 3 * N + 7) / 8 * 8;
  if (ensure_workspace(c, kSampleKeyBytes + small_bytes + count * per_ct_words * 8)) return 1;
  w.d_kb = c->ws;
  w.d_small = (int8_t *)c->ws + kSampleKeyBytes;
  w.u = (u64 *)(w.d_small + small_bytes);
  w.cfull = w.u + count * K * N;
  w.err = w.cfull + count * 2 * K * N;
  w.prodD = w.err + count * 2 * K * N;
  w.prodS = w.prodD + count * 2 * L * N;
  w.tmod = w.prodS + count * 2 * N;
  w.wipe_bytes = kSampleKeyBytes + small_bytes + count * 5 * K * N * 8;
  return 0;
}
// ciphertexts from the draws in w.d_small (u | e0 | e1 per ciphertext): everything downstream of the sampling
static int encrypt_from_small(abc_hip_ctx *c, const u64 *plain, u64 *ct, size_t count, const EncryptWs &w, bool wipe) {
  const size_t N = (size_t)c->n;
  const int K = c->K, L = c->L;
  const bool ckks = (c->scheme == 2);
  const int8_t *d_small = w.d_small;
  u64 *u = w.u, *cfull = w.cfull, *err = w.err, *prodD = w.prodD, *prodS = w.prodS, *tmod = w.tmod;
  LimbMap kmap{};
  for (int j = 0; j < K; j++) kmap.id[j] = j;
  // u (poly 0 of each [3][N] triple) -> residues at key level -> NTT
  hipLaunchKernelGGL(k_small_to_rns, dim3(grid_for(count * K * N, 256)), dim3(256), 0, c->stream, c->dc, d_small, (size_t)1, 3 * N,
                     (size_t)0, u, kmap, K, count);
  ABC_HIP_CHECK(hipGetLastError());
  if (launch_ntt_fwd(c, u, kmap, K, count * K)) return 1;
  // errors e0,e1 (polys 1,2 of each triple) -> residues [count][2][K][N]
  hipLaunchKernelGGL(k_small_to_rns, dim3(grid_for(count * 2 * K * N, 256)), dim3(256), 0, c->stream, c->dc, d_small, (size_t)2,
                     3 * N, N, err, kmap, K, count * 2);
  ABC_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_enc_mul_pk, dim3(grid_for(count * 2 * K * N, 256)), dim3(256), 0, c->stream, c->dc, u, c->d_pk, cfull, count);
  ABC_HIP_CHECK(hipGetLastError());
  if (ckks) {
    if (launch_ntt_fwd(c, err, kmap, K, count * 2 * K)) return 1;
  } else {
    if (launch_ntt_inv(c, cfull, kmap, K, count * 2 * K)) return 1;
  }
  hipLaunchKernelGGL(k_acc_add, dim3(grid_for(count * 2 * K * N, 256)), dim3(256), 0, c->stream, c->dc, cfull, err,
                     (size_t)K * N, kmap, K, count * 2);
  ABC_HIP_CHECK(hipGetLastError());
  // modulus switch key level -> data level (divide_and_round_q_last(_ntt)_inplace)
  if (split_special(c, cfull, prodD, prodS, count * 2)) return 1;
  LimbMap smap{};
  smap.id[0] = K - 1;
  if (ckks && launch_ntt_inv(c, prodS, smap, 1, count * 2)) return 1;
  if (launch_ks_tmod(c, prodS, tmod, L, count * 2)) return 1;
  const LimbMap dmap = key_limb_map(c, L);
  if (ckks && launch_ntt_fwd(c, tmod, dmap, L, count * 2 * L)) return 1;
  if (launch_ks_finish(c, prodD, tmod, ct, nullptr, 0, false, L, count)) return 1;
  // the encryption randomness (the sampling key, u, e0, e1 and everything derived before the modulus switch) lives in the
  // workspace: wipe it
  if (wipe) ABC_HIP_CHECK(hipMemsetAsync(c->ws, 0, w.wipe_bytes, c->stream));
  // add the message
  if (ckks) return ckks_add_plain(c, ct, plain, (size_t)L * N, ct, 2, L, count, 0);
  return bfv_addsub_plain(c, ct, plain, N, ct, 2, count, 0);
}
static int no_public_key(const abc_hip_ctx *c) {
  if (c->d_pk) return 0;
  set_error("encrypt: no public key (call abc_hip_keygen or abc_hip_load_public_key)");
  return 1;
}
// The seeded spec: ciphertext i draws u, e0, e1 from Rng(seed + i) -- independent streams, so a batch is drawn by up to 16 host
// threads and the bytes do not depend on the thread count.  Config 5 encrypts 1 125 ciphertexts of 2^16 slots: 221 M draws,
// 530 ms on one thread.
int encrypt(abc_hip_ctx *c, const u64 *plain, uint64_t seed, u64 *ct, size_t count) {
  if (no_public_key(c)) return 1;
  if (!count) return 0;
  const size_t N = (size_t)c->n;
  std::vector<int8_t> h_small(count * 3 * N);
  const size_t hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const size_t workers = count >= 4 ? std::min(hw, count) : 1;
  auto work = [&](size_t w) {
    for (size_t i = count * w / workers; i < count * (w + 1) / workers; i++) {
      Rng rng(seed + i);
      int8_t *p = h_small.data() + i * 3 * N;
      for (size_t x = 0; x < N; x++) p[x] = rng.ternary();
      for (size_t x = 0; x < 2 * N; x++) p[N + x] = rng.cbd();
    }
  };
  std::vector<std::thread> pool;
  for (size_t w = 1; w < workers; w++) pool.emplace_back(work, w);
  work(0);
  for (auto &t : pool) t.join();
  EncryptWs w;
  if (encrypt_workspace(c, count, w)) return 1;
  if (upload_wiped(c, w.d_small, h_small.data(), h_small.size())) return 1;
  return encrypt_from_small(c, plain, ct, count, w, false);
}
// The keyed spec: ciphertext i takes stream nonce + i; u from words 0 .. N-1 (ternary), e0 and e1 from the 2N words behind (cbd).
// The draws [count][3][N] of (key, nonce) into d_small: by the device sampler, which reads the key from d_kb (kSampleKeyBytes of
// device memory that the caller wipes), or under ABC_HIP_HOST_SAMPLING=1 by the host twin and an upload.
static int keyed_small_draws(abc_hip_ctx *c, const uint8_t key[32], uint64_t nonce, size_t count, void *d_kb, int8_t *d_small) {
  if (c->sw.host_sampling) {
    std::vector<int8_t> h_small(count * 3 * (size_t)c->n);
    keyed::encrypt_small_host(key, nonce, (size_t)c->n, count, h_small.data());
    return upload_wiped(c, d_small, h_small.data(), h_small.size());
  }
  return upload_sample_key(c, d_kb, key, nonce) || launch_sample_small(c, d_kb, 0, count, 3, 1, d_small);
}
int encrypt_keyed(abc_hip_ctx *c, const u64 *plain, const uint8_t key[32], uint64_t nonce, u64 *ct, size_t count) {
  if (!key) { set_error("encrypt_keyed: null key"); return 1; }
  if (no_public_key(c)) return 1;
  if (!count) return 0;
  EncryptWs w;
  if (encrypt_workspace(c, count, w)) return 1;
  if (keyed_small_draws(c, key, nonce, count, w.d_kb, w.d_small)) return 1;
  return encrypt_from_small(c, plain, ct, count, w, true);
}
int encrypt_secure(abc_hip_ctx *c, const u64 *plain, u64 *ct, size_t count) {
  uint8_t key[32];  // fresh per call, so every (key, nonce + i) pair is used once
  int rc = getrandom_fill(key, sizeof(key));
  if (rc) set_error("encrypt: getrandom failed");
  else rc = encrypt_keyed(c, plain, key, 0, ct, count);
  explicit_bzero(key, sizeof(key));
  return rc;
}
// the raw draws of the keyed spec, as encrypt_keyed takes them
int keyed_small(abc_hip_ctx *c, const uint8_t key[32], uint64_t nonce, int8_t *d_small, size_t count) {
  if (!key || (!d_small && count)) { set_error("keyed_small: null pointer"); return 1; }
  if ((uintptr_t)d_small & 7) { set_error("keyed_small: d_small must be 8-byte aligned"); return 1; }
  if (!count) return 0;
  if (ensure_workspace(c, kSampleKeyBytes)) return 1;
  const int rc = keyed_small_draws(c, key, nonce, count, c->ws, d_small);
  ABC_HIP_CHECK(hipMemsetAsync(c->ws, 0, kSampleKeyBytes, c->stream));
  return rc;
}
int keyed_uniform(abc_hip_ctx *c, const uint8_t key[32], uint64_t stream, int nkeys, u64 *d_a) {
  if (!key || !d_a) { set_error("keyed_uniform: null pointer"); return 1; }
  if (nkeys < 1 || nkeys > c->L) { set_error("keyed_uniform: nkeys must be between 1 and L"); return 1; }
  if ((uintptr_t)d_a & 15) { set_error("keyed_uniform: d_a must be 16-byte aligned"); return 1; }
  if (c->sw.host_sampling) {
    std::vector<uint64_t> h_a((size_t)nkeys * c->K * c->n);
    uint32_t k[8];
    keyed::load_key(key, k);
    sample_uniform_host(c, k, stream, nkeys, h_a.data());
    explicit_bzero(k, sizeof(k));
    return upload_wiped(c, d_a, h_a.data(), h_a.size() * 8);
  }
  if (ensure_workspace(c, kSampleKeyBytes)) return 1;
  const int rc = upload_sample_key(c, c->ws, key, 0) || launch_sample_uniform(c, c->ws, stream, nkeys, d_a);
  ABC_HIP_CHECK(hipMemsetAsync(c->ws, 0, kSampleKeyBytes, c->stream));
  return rc;
}

// ---------------- decryption ----------------
// phase = c0 + c1*s (+ c2*s^2) at the ciphertext's level
__global__ __launch_bounds__(256) void k_phase_mul(DevCtx c, const u64 *cn, const u64 *sk, u64 *acc, int size, int nl, size_t count) {
  // cn: [count][size-1][nl][N] NTT form of c1.. ; acc [count][nl][N]
  const size_t pw = (size_t)nl * c.n;
  const size_t items = count * pw;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t ct = it / pw, w = it % pw;
    const Mod m = c.mods[w >> c.logn];
    const u64 s = sk[w];
    u64 sp = s, sum = 0;
    for (int p = 1; p < size; p++) {
      sum = add_mod(sum, mul_mod(cn[(ct * (size - 1) + (p - 1)) * pw + w], sp, m), m.q);
      if (p + 1 < size) sp = mul_mod(sp, s, m);
    }
    acc[it] = sum;
  }
}

// c1 s (+ c2 s^2) of `count` ciphertexts into the workspace, coefficient form for BFV (forward NTT of c1.., product with the
// powers of s, inverse NTT), NTT form for CKKS; the caller adds c0.  `extra` bytes of workspace behind the accumulator are the
// caller's (*extra_out).
static int phase_without_c0(abc_hip_ctx *c, const u64 *ct, int size, int nl, size_t count, size_t extra, u64 **acc_out, void **extra_out) {
  const size_t N = (size_t)c->n;
  const bool ckks = (c->scheme == 2);
  const size_t pw = (size_t)nl * N;
  if (ensure_workspace(c, (count * (size - 1) * pw + count * pw) * 8 + extra)) return 1;
  u64 *cn = (u64 *)c->ws, *acc = cn + count * (size - 1) * pw;
  const LimbMap dmap = key_limb_map(c, nl);
  // copy c1.. (strided inside each ciphertext)
  ABC_HIP_CHECK(hipMemcpy2DAsync(cn, (size - 1) * pw * 8, ct + pw, size * pw * 8, (size - 1) * pw * 8, count,
                                 hipMemcpyDeviceToDevice, c->stream));
  if (!ckks && launch_ntt_fwd(c, cn, dmap, nl, count * (size - 1) * nl)) return 1;
  hipLaunchKernelGGL(k_phase_mul, dim3(grid_for(count * pw, 256)), dim3(256), 0, c->stream, c->dc, cn, c->d_sk, acc, size, nl,
                     count);
  ABC_HIP_CHECK(hipGetLastError());
  if (!ckks && launch_ntt_inv(c, acc, dmap, nl, count * nl)) return 1;
  *acc_out = acc;
  if (extra_out) *extra_out = acc + count * pw;
  return 0;
}

int decrypt(abc_hip_ctx *c, const u64 *ct, int size, int nl, u64 *plain, size_t count) {
  if (!c->d_sk) { set_error("decrypt: no secret key"); return 1; }
  if (size < 2 || size > 3) { set_error("decrypt: ciphertext size must be 2 or 3"); return 1; }
  if (!count) return 0;
  const size_t N = (size_t)c->n;
  const bool ckks = (c->scheme == 2);
  if (!ckks && nl != c->L) { set_error("decrypt: BFV ciphertexts live at the top level"); return 1; }
  const size_t pw = (size_t)nl * N;
  u64 *acc = nullptr;
  if (phase_without_c0(c, ct, size, nl, count, 0, &acc, nullptr)) return 1;
  const LimbMap dmap = key_limb_map(c, nl);
  // + c0
  u64 *dst = ckks ? plain : acc;
  if (ckks) ABC_HIP_CHECK(hipMemcpyAsync(plain, acc, count * pw * 8, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_acc_add, dim3(grid_for(count * pw, 256)), dim3(256), 0, c->stream, c->dc, dst, ct, (size_t)size * pw, dmap,
                     nl, count);
  ABC_HIP_CHECK(hipGetLastError());
  if (ckks) return 0;
  return launch_bfv_decrypt_round(c, acc, plain, count);
}

// ---------------- invariant noise budget (BFV) ----------------
// One thread per (ciphertext, coefficient): v = t (c0 + c1 s + c2 s^2) per limb (acc: the inverse-transformed c1 s + c2 s^2), the
// exact centred lift of v (abc_crt_lift.hpp), the bit length of its magnitude; the maximum over the wavefront by cross-lane
// shuffles, over the block's waves through LDS, then one atomicMax per block into bits[ciphertext] (zeroed before the launch).
// An integer maximum does not depend on the order of arrival.  N is a multiple of the block size (logn >= 10): no tail.
constexpr int kNoiseThreads = 256;

template <int NLW>
__global__ __launch_bounds__(kNoiseThreads) void k_noise_bits(DevCtx c, const u64 *__restrict__ acc, const u64 *__restrict__ ct,
                                                              size_t ct_stride, const CodecConst *__restrict__ k, int nl,
                                                              int *__restrict__ bits) {
  __shared__ int wave_max[kNoiseThreads / 64];
  const size_t N = (size_t)c.n;
  const size_t b = blockIdx.x >> (c.logn - 8);  // N / 256 blocks per ciphertext
  const size_t n = ((size_t)(blockIdx.x & ((1u << (c.logn - 8)) - 1u)) << 8) + threadIdx.x;
  const u64 *pa = acc + b * nl * N + n, *p0 = ct + b * ct_stride + n;
  const DevConst *cst = c.cst;
  asm volatile("" : "+v"(cst));  // as the lift's constants: vector loads, no SGPR pressure
  u64 x[NLW];
  crt_lift_centred<NLW>(
      c.mods, k, nl, [=](int j, const Mod &m) { return mul_mod(add_mod(pa[(size_t)j * N], p0[(size_t)j * N], m.q), cst->t_mod_q[j], m); }, x);
  int v = 0;
#pragma unroll
  for (int w = 0; w < NLW; ++w)
    if (x[w]) v = 64 * w + 64 - __clzll((long long)x[w]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kNoiseThreads / 64; ++w) v = max(v, wave_max[w]);
    atomicMax(bits + b, v);
  }
}

int noise_budget(abc_hip_ctx *c, const u64 *ct, int size, int nl, int *h_budget, size_t count) {
  if (c->scheme != 1) { set_error("noise_budget: the invariant noise budget is defined for BFV only (this is a CKKS context)"); return 1; }
  if (!c->d_sk) { set_error("noise_budget: no secret key"); return 1; }
  if (size < 2 || size > 3) { set_error("noise_budget: ciphertext size must be 2 or 3"); return 1; }
  if (nl != c->L) { set_error("noise_budget: BFV ciphertexts live at the top level (nl = L)"); return 1; }
  if (!count) return 0;
  if (!ct || !h_budget) { set_error("noise_budget: null pointer"); return 1; }
  const size_t blocks_per_ct = (size_t)c->n / kNoiseThreads;
  if (count > 0x7fffffffu / blocks_per_ct) { set_error("noise_budget: batch too large for one call"); return 1; }
  if (ensure_crt_const(c)) return 1;
  const size_t pw = (size_t)nl * c->n;
  u64 *acc = nullptr;
  void *extra = nullptr;
  if (phase_without_c0(c, ct, size, nl, count, count * sizeof(int), &acc, &extra)) return 1;
  int *d_bits = (int *)extra;
  ABC_HIP_CHECK(hipMemsetAsync(d_bits, 0, count * sizeof(int), c->stream));
  const dim3 grid((unsigned)(count * blocks_per_ct)), block(kNoiseThreads);
  const CodecConst *k = (const CodecConst *)c->d_crt;
  if (nl <= 4) hipLaunchKernelGGL(k_noise_bits<4>, grid, block, 0, c->stream, c->dc, acc, ct, (size_t)size * pw, k, nl, d_bits);
  else if (nl <= 8) hipLaunchKernelGGL(k_noise_bits<8>, grid, block, 0, c->stream, c->dc, acc, ct, (size_t)size * pw, k, nl, d_bits);
  else hipLaunchKernelGGL(k_noise_bits<16>, grid, block, 0, c->stream, c->dc, acc, ct, (size_t)size * pw, k, nl, d_bits);
  ABC_HIP_CHECK(hipGetLastError());
  ABC_HIP_CHECK(hipMemcpyAsync(h_budget, d_bits, count * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  const int qbits = host::prod_bitlen(std::vector<uint64_t>(c->primes.begin(), c->primes.begin() + c->L));
  for (size_t i = 0; i < count; ++i) h_budget[i] = std::max(0, qbits - h_budget[i] - 1);
  return 0;
}

}  // namespace abc
