/*
 * abc_hip.h -- C ABI of libabc_hip.so: the MI355X (gfx950) FHE runtime backend that replaces
 * Microsoft SEAL behind ABC's AbstractCiphertext / AbstractCiphertextFactory plugin surface.
 *
 * Every entry point names the reference interface it replaces (paths relative to the ABC tree).
 * Conventions
 *   - every function returns 0 on success, non-zero on error; abc_hip_last_error() gives the text
 *     (the C++ shim turns it into std::runtime_error, the reference's only error convention:
 *     src/runtime/SealCiphertext.cpp:40,137).
 *   - `d_` pointers are DEVICE pointers obtained from abc_hip_malloc (or any HIP allocation, e.g. a
 *     torch tensor's data_ptr); `h_` pointers are host pointers.
 *   - all residues are uint64; layouts are row-major
 *        ciphertext batch  [count][size][nl][N]   BFV: coefficient form, CKKS: NTT form
 *        BFV plaintext     [count][N]             coefficients mod t
 *        CKKS plaintext    [count][nl][N]         NTT form
 *        key-switch key    [L][2][L+1][N]         (decomposition limb, component, key-level limb), NTT form
 *     `count` independent ciphertexts are processed by one call (the batch dimension the reference's
 *     single-circuit RuntimeVisitor lacks, include/ast_opt/runtime/RuntimeVisitor.h:34).
 *   - work is enqueued on the context's stream (abc_hip_set_stream); results are observable after
 *     abc_hip_sync or any *_d2h copy.
 */
#ifndef ABC_HIP_H
#define ABC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABC_HIP_SCHEME_BFV 1  /* seal::scheme_type::bfv, src/runtime/SealCiphertextFactory.cpp:74 */
#define ABC_HIP_SCHEME_CKKS 2 /* HAVE_SEAL_CKKS, CMakeLists.txt:216 (no reference implementation) */

typedef struct abc_hip_ctx abc_hip_ctx;

const char *abc_hip_last_error(void);
int abc_hip_device_count(void);

/* ---- context: replaces SealCiphertextFactory::setupSealContext, SealCiphertextFactory.cpp:72-100 ----
 * primes = data limbs followed by the special key-switching prime (SEAL's key-level chain);
 * plain_modulus is ignored for CKKS. */
int abc_hip_ctx_create(int scheme, int logn, const uint64_t *h_primes, int nprimes, uint64_t plain_modulus, int device,
                       abc_hip_ctx **out);
void abc_hip_ctx_destroy(abc_hip_ctx *ctx);
/* seal::CoeffModulus::BFVDefault(N) (SealCiphertextFactory.cpp:80); returns the number of primes */
int abc_hip_default_bfv_primes(size_t n, uint64_t *h_out);
/* seal::PlainModulus::Batching(N, bits) (SealCiphertextFactory.cpp:83) */
uint64_t abc_hip_plain_modulus_batching(size_t n, int bits);
/* seal::CoeffModulus::Create(N, bit_sizes) ordering, for CKKS chains */
int abc_hip_create_primes(size_t n, const int *bit_sizes, int count, uint64_t *h_out);
/* 0 scheme, 1 logn, 2 nprimes, 3 L, 4 device, 5 BEHZ Bsk size, 6 device buffers held back for live graphs (scratch arenas,
 * keys and key mirrors that were replaced or dropped while a graph that owns them is alive; parked abc_hip_malloc blocks are not
 * counted); -1 for an unknown `what` */
int abc_hip_ctx_info(const abc_hip_ctx *ctx, int what);
/* Every operation of the context is enqueued on `hip_stream` from now on.  NULL does NOT mean HIP's legacy default
 * stream: it selects the context's own private non-blocking stream again (the state after abc_hip_ctx_create), which is
 * not ordered against anything else -- a caller that produces inputs on another stream (e.g. torch's current stream, whose
 * handle is 0 for the default stream) must synchronise that stream before the call and abc_hip_sync after it, or pass a
 * real stream handle here (bench.py creates a torch.cuda.Stream and passes its handle). */
int abc_hip_set_stream(abc_hip_ctx *ctx, void *hip_stream);
int abc_hip_sync(abc_hip_ctx *ctx);
/* The ABC_HIP_* path switches (README) are read when the context is created, not per operation; this re-reads them
 * (drains the stream first).  For A/B timing and the parity tests of the fallback paths. */
int abc_hip_ctx_reload_env(abc_hip_ctx *ctx);
/* Which kernel sequence a call of `count` ciphertexts at level nl takes (the route table: DESIGN.md section 3b), written
 * to buf as a short string such as "split14 front=lean pack=1 main=split4"; per-chunk fields are those of the first
 * chunk.  in_place: d_out aliases d_in (rotate, rescale).  Read-only: allocates nothing, launches nothing, touches no
 * stream (legal inside abc_hip_graph_begin..end).  nl is checked as the operation itself checks it (BFV: nl = L for every
 * op, multiply included; rescale and multiply_plain_rescale: CKKS and nl >= 2).  Non-zero on a bad op / nl or a buffer too small (80 bytes hold any). */
#define ABC_HIP_ROUTE_MUL_RELIN 0
#define ABC_HIP_ROUTE_KEYSWITCH 1 /* relinearize, keyswitch */
#define ABC_HIP_ROUTE_ROTATE 2    /* one Galois element */
#define ABC_HIP_ROUTE_RESCALE 3
#define ABC_HIP_ROUTE_MULTIPLY 4
#define ABC_HIP_ROUTE_ROTATE_ADD 5 /* one Galois element plus a second ciphertext; in_place: d_out aliases d_in */
#define ABC_HIP_ROUTE_ROTATE_MAC_PLAIN 7 /* CKKS: addend + plaintext (.) one Galois element; in_place: d_out aliases d_in (6 is unassigned) */
#define ABC_HIP_ROUTE_MULTIPLY_PLAIN_RESCALE 10 /* CKKS, nl >= 2: the rescale's route plus mulplain=fused / mulplain=separate (8 and 9 are unassigned) */
#define ABC_HIP_ROUTE_MUL_SUM_RELIN 12 /* relinearize(sum of products): the key switch's route plus tensor=sum / tensor=per_term; per-chunk fields: the first group's (11 is unassigned) */
#define ABC_HIP_ROUTE_DIAG_MATVEC_BSGS 13 /* CKKS: the baby rotation's route (as ABC_HIP_ROUTE_ROTATE, out of place), macsum=kernel / macsum=per_term, then the giant step's add=fused / add=separate; per-chunk fields: the first group's */
#define ABC_HIP_ROUTE_BFV_PLAIN_SUM 14 /* BFV: plainsum=fused / plainsum=ntt_domain for abc_hip_bfv_multiply_plain_sum of `count` ciphertexts */
#define ABC_HIP_ROUTE_BFV_MATVEC_BSGS 15 /* BFV: the baby rotation's route (as ABC_HIP_ROUTE_ROTATE, out of place), the plainsum= of an inner sum, then the giant step's add=fused / add=separate; per-chunk fields and the group: those of a one-step baby list */
#define ABC_HIP_ROUTE_PLAIN_SUM_RESCALE 16 /* CKKS, nl >= 2: the rescale's route plus sumrescale=fused / sumrescale=separate, for a sum of up to four terms over `count` size-2 ciphertexts (a longer sum is separate unless ABC_HIP_PLAIN_SUM_RESCALE_TERMS is set) */
#define ABC_HIP_ROUTE_CONST_SUM_RESCALE 18 /* CKKS, nl >= 2: the rescale's route plus constsum=fused / constsum=separate, for a one-term sum over `count` size-2 ciphertexts at nl (more than four terms or a term above nl: separate) */
#define ABC_HIP_ROUTE_POLY_EVAL 19 /* CKKS, nl >= 2: the mul_relin route at nl, then constsum=separate: the string answers for degree 2 and above, whose last step reads powers above its level; a degree-1 call has one term, at nl, and its last step takes what ABC_HIP_ROUTE_CONST_SUM_RESCALE says at nl (abc_hip_route has no argument for the degree) */
#define ABC_HIP_ROUTE_DIAG_MATVEC_BSGS_RESCALE 17 /* CKKS, nl >= 2: the baby rotation's route at nl, sumrescale=, then the giant step's route at nl - 1 with add=fused / add=separate; per-chunk fields: the first group's.  Two key-switch routes in one string: 160 bytes hold any */
int abc_hip_route(abc_hip_ctx *ctx, int op, int nl, size_t count, int in_place, char *buf, size_t cap);

/* ---- device memory (so that FFI callers need no HIP runtime binding) ----
 * Freed buffers are cached per context and recycled by size, so a buffer may be freed right after the last operation
 * on it has been issued, without synchronising; it must only be used with the context that allocated it.
 * ABC_HIP_SYNC_ALLOC=1 selects plain hipMalloc / synchronise + hipFree. */
int abc_hip_malloc(abc_hip_ctx *ctx, void **d_ptr, size_t bytes);
int abc_hip_free(abc_hip_ctx *ctx, void *d_ptr);
/* hand every cached (freed, not yet reused) buffer back to the driver; also done automatically when a device
 * allocation of this context fails and when the cache reaches its cap (a quarter of the device) */
int abc_hip_trim(abc_hip_ctx *ctx);
size_t abc_hip_cached_bytes(abc_hip_ctx *ctx);
int abc_hip_memcpy_h2d(abc_hip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int abc_hip_memcpy_d2h(abc_hip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* seal::Ciphertext copy-ctor = SealCiphertext::clone, src/runtime/SealCiphertext.cpp:13-16,71-78 */
int abc_hip_memcpy_d2d(abc_hip_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);

/* ---- keys: replaces seal::KeyGenerator use at SealCiphertextFactory.cpp:89-93 ---- */
/* generate sk, pk, relin key and all default Galois keys on the device.
 * abc_hip_keygen_secure: what a deployment uses (and HipCiphertextFactory's default): secret key and errors from ChaCha20
 * keyed with 256 bits of getrandom(2), the published uniform polynomials from an independently keyed stream, drawn on the
 * device (abc_hip_keygen_keyed below), secret temporaries wiped before release.
 * abc_hip_keygen(seed): TEST ONLY -- the repo's reproducible sampling spec (splitmix64-seeded xoshiro256**),
 * which the CPU oracle implements too so that keys are bit-comparable; a 64-bit seed and a linear generator are not
 * cryptographic strength. */
int abc_hip_keygen_secure(abc_hip_ctx *ctx);
int abc_hip_keygen(abc_hip_ctx *ctx, uint64_t seed);
/* The keyed sampling spec ("Keyed sampling spec"): counter-based ChaCha20, every draw a pure function of
 * (key, stream id, word number), drawn by HIP kernels.  key_sec serves the secret key and the errors, key_pub the published
 * uniform polynomials; stream 0 the secret key, 1 the public key, 2 the relinearisation key, 2 + galois_elt a Galois key.
 * Deterministic given the two keys.  abc_hip_keygen_secure is this call with two fresh 32-byte keys from getrandom(2).
 * ABC_HIP_HOST_SAMPLING=1 draws the same words on the host (bit-identical keys); abc_hip_keygen_secure and
 * abc_hip_encrypt_secure are the keyed entries under keys from getrandom(2) and follow that switch with them.  Keys are rewritten
 * in place (graphs). */
int abc_hip_keygen_keyed(abc_hip_ctx *ctx, const uint8_t key_sec[32], const uint8_t key_pub[32]);
/* or load externally generated keys (host pointers) */
int abc_hip_load_secret_key(abc_hip_ctx *ctx, const uint64_t *h_sk /*[L+1][N] NTT*/);
int abc_hip_load_public_key(abc_hip_ctx *ctx, const uint64_t *h_pk /*[2][L+1][N]*/);
int abc_hip_load_relin_key(abc_hip_ctx *ctx, const uint64_t *h_key /*[L][2][L+1][N]*/);
int abc_hip_load_galois_key(abc_hip_ctx *ctx, uint32_t galois_elt, const uint64_t *h_key);
int abc_hip_get_secret_key(abc_hip_ctx *ctx, uint64_t *h_out);
int abc_hip_get_public_key(abc_hip_ctx *ctx, uint64_t *h_out);
int abc_hip_get_relin_key(abc_hip_ctx *ctx, uint64_t *h_out);
int abc_hip_get_galois_key(abc_hip_ctx *ctx, uint32_t galois_elt, uint64_t *h_out);
int abc_hip_num_galois_keys(abc_hip_ctx *ctx);
uint32_t abc_hip_galois_elt_at(abc_hip_ctx *ctx, int i);
uint32_t abc_hip_galois_elt_from_step(abc_hip_ctx *ctx, int step);

/* ---- encode / encrypt / decrypt / decode ----
 * seal::BatchEncoder::encode (SealCiphertextFactory.cpp:130): d_values int64 [count][N] (already padded
 * by the caller as SealCiphertextFactory::expandVector does, :102-115) -> d_plain [count][N] */
int abc_hip_batch_encode(abc_hip_ctx *ctx, const int64_t *d_values, uint64_t *d_plain, size_t count);
/* seal::BatchEncoder::decode (SealCiphertextFactory.cpp:151) */
int abc_hip_batch_decode(abc_hip_ctx *ctx, const uint64_t *d_plain, int64_t *d_values, size_t count);
/* CKKS counterpart of seal::BatchEncoder::encode (SealCiphertextFactory.cpp:130; no reference CKKS implementation, see
 * ABC_HIP_SCHEME_CKKS): d_re / d_im (d_im may be NULL = real slots) [count][values_per_row] doubles, values_per_row <= N/2,
 * the rest of the N/2 slots zero -> d_plain [count][nl][N], NTT form (ready for abc_hip_encrypt / *_plain), limb j modulo q_j.
 * Slot i is the evaluation at zeta^(3^i), zeta = exp(i pi / N) (the order of runtime/CkksEncoder.hpp).  Coefficients are rounded to the
 * nearest integer, ties away from zero (SEAL's rule, the one of abc_hip_ckks_const_words and of both host encoders: 0.5 -> 1,
 * -0.5 -> -1, 2.5 -> 3); one reaching 2^62 in magnitude after rounding, or a value that is not finite, fails the call with status 2.
 * Reads one word back: not capturable. */
int abc_hip_ckks_encode(abc_hip_ctx *ctx, const double *d_re, const double *d_im, size_t values_per_row, double scale,
                        int nl, uint64_t *d_plain, size_t count);
/* CKKS counterpart of seal::BatchEncoder::decode (SealCiphertextFactory.cpp:151; no reference CKKS implementation):
 * d_plain [count][nl][N] NTT form (as abc_hip_decrypt writes it; not modified) -> d_re / d_im (d_im may be NULL)
 * [count][N/2] slot values divided by scale, from the exact centred lift into (-Q/2, Q/2], Q = q_0 ... q_{nl-1}.
 * Not capturable. */
int abc_hip_ckks_decode(abc_hip_ctx *ctx, const uint64_t *d_plain, int nl, double scale, double *d_re, double *d_im,
                        size_t count);
/* seal::Encryptor::encrypt, public key (SealCiphertextFactory.cpp:12).
 * abc_hip_encrypt_secure: encryption randomness from a freshly OS-keyed ChaCha20 stream per call (never derived from a
 * key seed), wiped afterwards.  abc_hip_encrypt(seed): TEST ONLY, ciphertext i uses the reproducible stream seed+i. */
int abc_hip_encrypt_secure(abc_hip_ctx *ctx, const uint64_t *d_plain, uint64_t *d_ct, size_t count);
int abc_hip_encrypt(abc_hip_ctx *ctx, const uint64_t *d_plain, uint64_t seed, uint64_t *d_ct, size_t count);
/* Keyed sampling spec: ciphertext i draws u, e0, e1 from ChaCha20 stream nonce + i (mod 2^64) of `key`, on the device; the key
 * and the draws are wiped afterwards.  abc_hip_encrypt_secure is this call with a fresh key from getrandom(2) and nonce 0.
 * Deterministic given (key, nonce): the caller must never reuse a (key, nonce + i) pair. */
int abc_hip_encrypt_keyed(abc_hip_ctx *ctx, const uint64_t *d_plain, const uint8_t key[32], uint64_t nonce, uint64_t *d_ct,
                          size_t count);
/* the raw draws, for parity tests: d_small int8 [count][3][N] (u | e0 | e1), 8-byte aligned */
int abc_hip_keyed_small(abc_hip_ctx *ctx, const uint8_t key[32], uint64_t nonce, int8_t *d_small, size_t count);
/* d_a u64 [nkeys][K][N], stream id as in the spec, 1 <= nkeys <= L, 16-byte aligned */
int abc_hip_keyed_uniform(abc_hip_ctx *ctx, const uint8_t key[32], uint64_t stream, int nkeys, uint64_t *d_a);
/* host twin of abc_hip_keyed_small, no context and no GPU: h_small int8 [count][3][n], n a multiple of 8 */
int abc_hip_keyed_small_host(const uint8_t key[32], uint64_t nonce, size_t n, size_t count, int8_t *h_small);
/* seal::Decryptor::decrypt (SealCiphertextFactory.cpp:150); size = 2 or 3 polynomials */
int abc_hip_decrypt(abc_hip_ctx *ctx, const uint64_t *d_ct, int size, int nl, uint64_t *d_plain, size_t count);
/* Decryptor::invariant_noise_budget (SealCiphertext.cpp:80-83): BFV only, secret key required, size = 2 or 3, nl = L.
 * d_ct [count][size][nl][N] coefficient form -> h_budget [count] HOST ints, one per ciphertext:
 *   v = t (c0 + c1 s + c2 s^2) mod Q, Q = q_0 ... q_{L-1}, lifted coefficient-wise into (-Q/2, Q/2] (exact, integers only);
 *   m = the largest |coefficient|; budget = max(0, bitlen(Q) - bitlen(m) - 1), bitlen(0) = 0.
 * A positive budget means the ciphertext still decrypts.  Everything runs on the device; the only transfer is the read-back of
 * `count` ints (one stream synchronisation): not capturable.  A CKKS context, a missing secret key, another size or another
 * level fail the call (non-zero status); count = 0 succeeds. */
int abc_hip_noise_budget(abc_hip_ctx *ctx, const uint64_t *d_ct, int size, int nl, int *h_budget, size_t count);

/* ---- evaluator: replaces the seal::Evaluator calls in src/runtime/SealCiphertext.cpp ---- */
/* Evaluator::add / add_inplace (:92,:114) */
int abc_hip_add(abc_hip_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, int size, int nl, size_t count);
/* Evaluator::sub / sub_inplace (:98,:118) */
int abc_hip_sub(abc_hip_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, int size, int nl, size_t count);
/* Evaluator::negate / negate_inplace (:157,:193) */
int abc_hip_negate(abc_hip_ctx *ctx, const uint64_t *d_a, uint64_t *d_out, int size, int nl, size_t count);
/* Evaluator::multiply(_inplace) (:104,:122): size-2 x size-2 -> size-3, no relinearisation */
int abc_hip_multiply(abc_hip_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out3, int nl, size_t count);
/* Evaluator::relinearize_inplace (:105,:123,:160,:197): size-3 -> size-2 */
int abc_hip_relinearize(abc_hip_ctx *ctx, const uint64_t *d_ct3, uint64_t *d_out2, int nl, size_t count);
/* SealCiphertext::multiply / multiplyInplace = multiply + relinearize (:102-107,:121-124) -- THE hot path */
int abc_hip_mul_relin(abc_hip_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, int nl, size_t count);
/* A sum of ciphertext products with ONE relinearisation (lazy relinearisation): replaces n_terms x Evaluator::multiply (:104,:122),
 * n_terms - 1 x Evaluator::add (:92,:114) on the size-3 products, and -- abc_hip_mul_sum_relin -- one Evaluator::relinearize_inplace
 * (:105,:123) in place of one per product.
 *   abc_hip_multiply_sum:   d_out3 [count][3][nl][N] = a_0 (x) b_0 + ... + a_{K-1} (x) b_{K-1}, no relinearisation;
 *   abc_hip_mul_sum_relin:  d_out  [count][2][nl][N] = relinearize(that sum).
 * h_a, h_b: HOST arrays of n_terms device pointers, each [count][2][nl][N]; read during the call only.  h_a[k] == h_b[k] (a square)
 * and one pointer in several terms are fine.  Both calls are bit-identical to abc_hip_multiply per term, abc_hip_add at size 3 and
 * (the second) abc_hip_relinearize; n_terms == 1 gives the words of abc_hip_multiply / abc_hip_mul_relin.  The result of the second
 * call decrypts to what the sum of n_terms abc_hip_mul_relin results decrypts to, with one key switch's noise instead of n_terms;
 * its WORDS differ from that sum.  CKKS forms the size-3 sum with one K-term kernel (abc_hip_route,
 * ABC_HIP_ROUTE_MUL_SUM_RELIN: tensor=sum; the term pointers travel in the kernel's arguments, eight per launch); BFV, whose
 * product rounds (BEHZ), and ABC_HIP_NO_TENSOR_SUM=1 form each product on its own in a second arena and add (tensor=per_term).
 * abc_hip_mul_sum_relin keeps the sum in a context arena and walks the batch in groups of ciphertexts (a multiple of the key
 * switch's chunk * lanes, the arena capped at 4 GiB; with ABC_HIP_CHUNK=c exactly c * lanes), so d_out may BE one of the terms.
 * n_terms == 0 writes zeros; count == 0 succeeds and enqueues nothing.  Fails with nothing written or enqueued for: n_terms < 0, a
 * null term pointer, a bad level (BFV: nl = L), no relinearisation key (second call), d_out3 overlapping a term, d_out overlapping
 * a term without being exactly that term's pointer.  Capturable, under the "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_multiply_sum(abc_hip_ctx *ctx, const uint64_t *const *h_a, const uint64_t *const *h_b, int n_terms, uint64_t *d_out3,
                         int nl, size_t count);
int abc_hip_mul_sum_relin(abc_hip_ctx *ctx, const uint64_t *const *h_a, const uint64_t *const *h_b, int n_terms, uint64_t *d_out,
                          int nl, size_t count);
/* Evaluator::rotate_rows(_inplace) (:55,:60), incl. SEAL's NAF decomposition for steps without a key */
int abc_hip_rotate(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int nl, int steps, size_t count);
/* Evaluator::apply_galois for one element */
int abc_hip_apply_galois(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int nl, uint32_t galois_elt, size_t count);
/* Several Galois elements of ONE input in one call, in the HOISTED FORM of a rotation (definition, and why this form: DESIGN.md
 * section 4).  d_in [count][2][nl][N] -> d_out [n_elts][count][2][nl][N], for an odd g = h_elts[r] < 2N with a Galois key:
 *   out[r] = ( s_g(ks0 + c0), s_g(ks1) ),  (ks0, ks1) = KeySwitch(c1, key'_g),
 * s_g the automorphism x -> x^g in the ciphertext's own form (NTT-index permutation for CKKS, coefficient permutation with
 * sign for BFV), key'_g the key of g with every [N] row permuted by g^-1 mod 2N in NTT form (a device mirror of the key, built
 * on first use).  The key switch runs on the UNPERMUTED c1, so its decomposition does not depend on g.  The result decrypts to
 * the same plaintext as abc_hip_apply_galois's, with the same noise distribution; it is NOT bit-identical to it.
 * GROUNDWORK, NOT A FAST PATH: the kernels do not share the decomposition between the elements yet.  Each element costs a whole key
 * switch and a permutation pass, measured 16 % SLOWER than the same number of abc_hip_rotate calls, and one
 * more key-sized device buffer per element used.  Call abc_hip_rotate unless this form itself is what is wanted.
 * Duplicate elements are allowed, each gets its own slab; n_elts == 0 and count == 0 succeed and enqueue nothing.  Fails for an
 * even or out-of-range element, an element without a key, a bad level, or d_out overlapping d_in: nothing is then written to d_out
 * or to scratch (where a later step fails, allocation say, permuted keys of earlier elements may have been built: mirrors only).
 * h_elts is read during the call only.  Capturable, under the "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_apply_galois_hoisted(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int nl, const uint32_t *h_elts, int n_elts,
                                 size_t count);
/* The same for rotation steps, as abc_hip_rotate counts them; step 0 copies the input.  A step without a key of its own fails
 * ("Galois key not present"): a NAF chain is sequential and has nothing to hoist. */
int abc_hip_rotate_hoisted(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int nl, const int *h_steps, int n_steps,
                           size_t count);
/* Evaluator::rotate_rows (SealCiphertext.cpp:55,60) followed by Evaluator::add (:92,114) as one call:
 * d_out = d_addend + rotate(d_in, steps); all three [count][2][nl][N].  Bit-identical to abc_hip_rotate into a temporary followed by
 * abc_hip_add, under every aliasing of the three pointers.  Where the route allows it (abc_hip_route, ABC_HIP_ROUTE_ROTATE_ADD:
 * a folded rotation of the split sequences with d_out != d_in) the addend is one more operand of the key switch's last kernel;
 * otherwise the rotation lands in an arena and the add kernel follows.  Step 0: d_addend + d_in.  A step without a key of its
 * own runs its NAF chain as abc_hip_rotate does; only the last hop can take the addend.  Errors are those of abc_hip_rotate, found
 * before anything is written.  Capturable, under the "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_rotate_add(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_addend, uint64_t *d_out, int nl, int steps,
                       size_t count);
/* the same for one Galois element (2N - 1: conjugation / column swap) */
int abc_hip_apply_galois_add(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_addend, uint64_t *d_out, int nl,
                             uint32_t galois_elt, size_t count);
/* The rotate-and-sum tree: acc = in; for each step s in order: acc = acc + rotate(acc, s); out = acc.  Every step is checked before
 * the first launch; the intermediate sums live in arenas and only the last one lands in d_out, which may be d_in.  n_steps == 0
 * copies.  h_steps is read during the call only.  Capturable like abc_hip_rotate_add. */
int abc_hip_rotate_sum(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int nl, const int *h_steps, int n_steps, size_t count);
/* CKKS only: Evaluator::rotate_vector, multiply_plain and add as one call, the term of a matrix-vector product by diagonals:
 * d_out = d_addend + d_plain (.) rotate(d_in, steps); the ciphertexts [count][2][nl][N], d_plain and plain_stride exactly as
 * abc_hip_multiply_plain takes them (0: one plaintext for the batch; >= nl * N: one per ciphertext, its first nl limbs read).
 * d_addend == NULL: no addend.  Bit-identical to abc_hip_rotate into a temporary, abc_hip_multiply_plain on it, then abc_hip_add
 * with the addend, under every aliasing of d_in, d_addend and d_out.  Where the route allows it (abc_hip_route,
 * ABC_HIP_ROUTE_ROTATE_MAC_PLAIN: a folded rotation of the N = 2^14 split sequence, or of the N = 2^15 one up to seven limbs, with
 * d_out != d_in) plaintext and addend are operands of the key switch's last kernel; otherwise the rotation lands in an arena,
 * the product is formed there and the add kernel follows.  No rescale: the result is at the scale of the product.  Step 0 has
 * no key switch: multiply_plain, then add.  A step without a key of its own runs its NAF chain as abc_hip_rotate does; only the
 * last hop takes the plaintext and the addend.  Fails for a BFV context, for d_plain overlapping d_out, and wherever
 * abc_hip_rotate or abc_hip_multiply_plain would; every error is found before anything is written.  Capturable, under the
 * "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_rotate_mac_plain(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_plain, size_t plain_stride,
                             const uint64_t *d_addend, uint64_t *d_out, int nl, int steps, size_t count);
/* the same for one Galois element (2N - 1: conjugation) */
int abc_hip_apply_galois_mac_plain(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_plain, size_t plain_stride,
                                   const uint64_t *d_addend, uint64_t *d_out, int nl, uint32_t galois_elt, size_t count);
/* CKKS only: a matrix-vector product by diagonals, d_out = sum over r of diag_r (.) rotate(d_in, h_steps[r]), accumulated in the
 * order given.  One set of diagonals for the whole batch: row r starts at d_diags + r * diag_stride, diag_stride >= nl * N words,
 * and its first nl limbs are read, so rows encoded at a higher level ([n_steps][L][N], stride L * N) apply at nl < L.  The running
 * sum lives in d_out: a step 0 term is a plain product, every other one abc_hip_rotate_mac_plain with d_addend == d_out.
 * Duplicate steps are allowed.  n_steps == 0 writes zeros; count == 0 succeeds and enqueues nothing.  Every step and every key is
 * checked before the first launch; d_out overlapping d_in or d_diags, a bad stride, a step without a key (or a NAF chain of
 * keys) or a BFV context fail the call with nothing written.  h_steps is read during the call only.  Capturable like
 * abc_hip_rotate_mac_plain. */
int abc_hip_diag_matvec(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_diags, size_t diag_stride, const int *h_steps,
                        int n_steps, uint64_t *d_out, int nl, size_t count);
/* CKKS only: a plaintext-weighted sum of ciphertexts as one call -- a linear layer with one ciphertext per feature, a convolution
 * over channels, the inner sum of a baby-step giant-step matvec.  Replaces n_terms x Evaluator::multiply_plain (:159,:196) and
 * n_terms x Evaluator::add (:92,:114):
 *   d_out [count][size][nl][N] = (d_addend or 0) + plain_0 (.) ct_0 + ... + plain_{K-1} (.) ct_{K-1},  size = 2 or 3.
 * h_ct, h_plain: HOST arrays of n_terms device pointers, read during the call only; ct_k is [count][size][nl][N], and every plain_k
 * takes plain_stride exactly as abc_hip_multiply_plain does (0: one plaintext per term for the whole batch; >= nl * N: one per
 * ciphertext, its first nl limbs read, so rows encoded at a higher level apply at nl < L).  One pointer may appear in several
 * terms.  d_addend == NULL: no addend; d_out may be exactly d_addend.  Bit-identical to abc_hip_multiply_plain per term and
 * abc_hip_add in any order: the sums are exact and canonical.  One K-term kernel forms the sum (abc_hip_route,
 * ABC_HIP_ROUTE_DIAG_MATVEC_BSGS: macsum=kernel; the term pointers travel in the kernel's arguments, eight per launch, and the
 * running sum is carried by pointer from launch to launch); ABC_HIP_NO_PLAIN_MAC_SUM=1 forms each product on its own in an arena
 * and adds (macsum=per_term).  n_terms == 0 writes the addend, or zeros without one; count == 0 succeeds and enqueues nothing.
 * Fails with nothing written or enqueued for: a BFV context, a bad level, size or stride, n_terms < 0, a null term pointer, d_out
 * overlapping any ct_k or plain_k, d_out overlapping d_addend without being equal to it.  Capturable, under the "run once eagerly
 * first" rule of abc_hip_graph_begin. */
int abc_hip_multiply_plain_sum(abc_hip_ctx *ctx, const uint64_t *const *h_ct, const uint64_t *const *h_plain, size_t plain_stride,
                               int n_terms, const uint64_t *d_addend, uint64_t *d_out, int size, int nl, size_t count);
/* CKKS only: the slot rotation of PLAINTEXTS, d_plain [rows][nl][N] in NTT form -> d_out likewise: the index permutation
 * Evaluator::rotate_rows (:55,:60) applies to either component of a ciphertext, with no key and no key switch.  Negative steps
 * rotate the other way; step 0 is a copy.  rotate_plain(encode(v), s) is encode(v rotated by s), word for word.  Fails for a BFV
 * context, a bad level, |steps| >= N / 2, or d_out overlapping d_plain.  Capturable. */
int abc_hip_rotate_plain(abc_hip_ctx *ctx, const uint64_t *d_plain, uint64_t *d_out, int nl, int steps, size_t rows);
/* CKKS only: a matrix-vector product by diagonals, baby-step giant-step: n_baby + n_giant rotations serve n_baby * n_giant
 * diagonals, where abc_hip_diag_matvec pays one key switch per diagonal.
 *   d_out = sum over j of rotate( sum over i of D[j * n_baby + i] (.) rotate(d_in, h_baby[i]),  h_giant[j] ).
 * Row (j, i) of D starts at d_diags + (j * n_baby + i) * diag_stride; diag_stride >= nl * N and the first nl limbs are read; one
 * set for the batch, as in abc_hip_diag_matvec.  THE CALLER SUPPLIES ROWS ALREADY ROTATED BY -h_giant[j]:
 *   D[j, i] = rotate_plain(diag_{h_giant[j] + h_baby[i]}, -h_giant[j]),
 * because  diag (.) rot(rot(x, b), g) = rot( rot_plain(diag, -g) (.) rot(x, b), g ):  a rotation distributes over the slot-wise
 * product, so the giant rotation can be taken once, behind the inner sum (abc_hip_rotate_plain does the pre-rotation).
 * Sequence: the baby rotations run as abc_hip_rotate does (Evaluator::rotate_rows :55,:60; NAF chains included; step 0 is d_in
 * itself) into an arena; per giant step one abc_hip_multiply_plain_sum (Evaluator::multiply_plain :159,:196, add :92,:114) over
 * the n_baby rotated ciphertexts lands in a second arena; then d_out = d_out + rotate(inner_j, h_giant[j]) as abc_hip_rotate_add
 * does, fused where its route says so.  A giant step of 0 is a plain add; the first j writes d_out.  Order is as given,
 * duplicates are allowed.  The batch is walked in groups of ciphertexts that keep the baby arena within 4 GiB (the rule of
 * abc_hip_mul_sum_relin; with ABC_HIP_CHUNK=c exactly c * lanes).  n_baby == 0 or n_giant == 0 writes zeros; count == 0 succeeds
 * and enqueues nothing.  Every step and every key is checked before the first launch; a BFV context, a bad level or stride, a
 * negative count, a null step list, a step without a key (or a NAF chain of keys), d_out overlapping d_in or d_diags fail the call
 * with nothing written.  The step lists are read during the call only.  Capturable like abc_hip_rotate_add. */
int abc_hip_diag_matvec_bsgs(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_diags, size_t diag_stride, const int *h_baby,
                             int n_baby, const int *h_giant, int n_giant, uint64_t *d_out, int nl, size_t count);
/* CKKS only, nl >= 2: a plaintext-weighted sum with ONE rescale behind it (a linear layer):
 *   d_out [count][size][nl-1][N] = rescale( (d_addend or 0) + plain_0 (.) ct_0 + ... + plain_{K-1} (.) ct_{K-1} ),  size = 2 or 3.
 * Operands exactly as abc_hip_multiply_plain_sum takes them; d_addend is [count][size][nl][N].  Bit-identical to
 * abc_hip_multiply_plain_sum into a temporary followed by abc_hip_rescale; n_terms == 1 without an addend gives the words of
 * abc_hip_multiply_plain_rescale.  The same VALUES as a rescale per product, with one rescale rounding instead of K -- other words.
 * Route (abc_hip_route, ABC_HIP_ROUTE_PLAIN_SUM_RESCALE): sumrescale=fused -- the K-term forms of the two LDS-resident rescale
 * kernels (rings 2^10 .. 2^14) form the sum in their loads, so it never reaches memory -- or sumrescale=separate -- the whole sum
 * into a context arena by the K-term kernel of abc_hip_multiply_plain_sum, then the rescale: N >= 2^15, ABC_HIP_NO_FUSED=1,
 * ABC_HIP_NO_ISPLIT=1 on a chain with a prime above 2^50, ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION=1, ABC_HIP_NO_PLAIN_MAC_SUM=1, and
 * where the measurement has the two steps as fast or faster: more than four terms, fewer than 256 polynomials (count * size) or
 * fewer than 2^20 coefficients among them.  ABC_HIP_PLAIN_SUM_RESCALE_TERMS=t (0 .. 8) fuses at every batch and term count: the
 * pair takes the last t terms at most and the sum of the others, formed in the arena, as its carry.  n_terms == 0
 * writes the rescaled addend, or zeros without one; count == 0 succeeds and enqueues nothing.  Fails with nothing written or
 * enqueued for: a BFV context, nl < 2 or a bad level, size or stride, n_terms < 0, a null term pointer, d_out overlapping any ct_k,
 * plain_k or d_addend (the shapes differ: equality is no exception).  Capturable, under the "run once eagerly first" rule of
 * abc_hip_graph_begin. */
int abc_hip_multiply_plain_sum_rescale(abc_hip_ctx *ctx, const uint64_t *const *h_ct, const uint64_t *const *h_plain, size_t plain_stride,
                                       int n_terms, const uint64_t *d_addend, uint64_t *d_out, int size, int nl, size_t count);
/* CKKS only, nl >= 2: abc_hip_diag_matvec_bsgs with every inner sum rescaled BEFORE its giant rotation:
 *   d_out [count][2][nl-1][N] = sum over j of rotate( rescale( sum over i of D[j * n_baby + i] (.) rotate(d_in, h_baby[i]) ),  h_giant[j] ).
 * The n_giant key switches of the giant steps run at nl - 1 limbs and the result arrives rescaled: another ciphertext than
 * abc_hip_rescale(abc_hip_diag_matvec_bsgs(...)), word for word, that decrypts to the same values.  Rows pre-rotated and laid out as
 * for abc_hip_diag_matvec_bsgs (nl limbs are read).  Sequence: the baby rotations at nl into an arena; per giant step one
 * abc_hip_multiply_plain_sum_rescale into a second arena; then d_out = d_out + rotate(inner_j, h_giant[j]) at nl - 1 as
 * abc_hip_rotate_add does.  A giant step of 0 writes d_out directly where it is the first, else abc_hip_add adds it.  Bit-identical
 * to that sequence of calls.  Order, duplicates, groups, empty lists, count == 0, the checks before the first launch and the
 * refusals as in abc_hip_diag_matvec_bsgs, and nl < 2.  Route: ABC_HIP_ROUTE_DIAG_MATVEC_BSGS_RESCALE.  Capturable like
 * abc_hip_rotate_add. */
int abc_hip_diag_matvec_bsgs_rescale(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_diags, size_t diag_stride, const int *h_baby,
                                     int n_baby, const int *h_giant, int n_giant, uint64_t *d_out, int nl, size_t count);
/* ---- BFV: plaintext-weighted sums with ONE inverse transform ----
 * A BFV Evaluator::multiply_plain (:159,:196) is INTT(NTT(ct) (.) NTT(lift(plain))) per limb.  The inverse transform is linear and
 * every step is exact modulo q_i, so a weighted sum is accumulated in NTT form and inverted once, with weights transformed once. */
/* Evaluator::transform_to_ntt(plain): d_plain [rows][N] mod t -> d_plain_ntt [rows][L][N]: the lift multiply_plain applies
 * (values of (t + 1) / 2 and above move up by q_i - t) and the forward transform per data limb.  BFV only; d_plain_ntt must not
 * overlap d_plain; rows == 0 enqueues nothing.  Capturable. */
int abc_hip_bfv_plain_to_ntt(abc_hip_ctx *ctx, const uint64_t *d_plain, uint64_t *d_plain_ntt, size_t rows);
#define ABC_HIP_CT_COEFF 0 /* terms as BFV ciphertexts travel everywhere else */
#define ABC_HIP_CT_NTT 1   /* terms already transformed limb by limb (abc_hip_ntt_limbs, nl = L): Evaluator::transform_to_ntt_inplace */
/* BFV only: replaces n_terms x Evaluator::multiply_plain (:159,:196) and n_terms x Evaluator::add (:92,:114):
 *   d_out [count][size][L][N], coefficient form = (d_addend or 0) + plain_0 * ct_0 + ... + plain_{K-1} * ct_{K-1},  size = 2 or 3.
 * h_ct, h_plain_ntt: HOST arrays of n_terms device pointers, read during the call only; ct_k is [count][size][L][N] in the form
 * ct_form says, plain_k in NTT form as abc_hip_bfv_plain_to_ntt writes it: [L][N] for the whole batch (plain_stride 0) or
 * [count][L][N] (plain_stride L * N).  One pointer may appear in several terms.  d_addend == NULL: no addend; d_out may be exactly
 * d_addend; addend and output are always coefficient form.  With ct_form == ABC_HIP_CT_COEFF the result is bit-identical to
 * abc_hip_multiply_plain per term and abc_hip_add in any order, and n_terms == 1 gives the words of abc_hip_multiply_plain: the sums
 * are exact and canonical.  Route (abc_hip_route, ABC_HIP_ROUTE_BFV_PLAIN_SUM): plainsum=fused -- rings 2^10 .. 2^14 with every
 * data prime below 2^50: one kernel transforms the terms of a limb in LDS, sums the products in registers and inverts once; the
 * term pointers travel in the kernel's arguments, eight per launch, and an NTT-domain partial sum in a context arena connects the
 * launches -- or plainsum=ntt_domain -- N >= 2^15, a prime of 2^50 or above, ABC_HIP_NO_FUSED=1, and at N = 2^14 a batch of at most
 * 48 limbs (count * 2 * L): stand-alone transforms into an arena, the K-term kernel of abc_hip_multiply_plain_sum, one inverse
 * transform, one add.  With ABC_HIP_CT_NTT neither route runs a forward transform.  The batch is walked in groups that keep the
 * arenas within 4 GiB.  n_terms == 0 writes the addend, or zeros without one; count == 0 succeeds and enqueues nothing.  Fails with
 * nothing written or enqueued for: a CKKS context, a size other than 2 or 3, a stride other than 0 or L * N, a ct_form other than
 * 0 or 1, n_terms < 0, a null term pointer, d_out overlapping any ct_k or plain_k, d_out overlapping d_addend without being equal
 * to it.  Capturable, under the "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_bfv_multiply_plain_sum(abc_hip_ctx *ctx, const uint64_t *const *h_ct, int ct_form, const uint64_t *const *h_plain_ntt,
                                   size_t plain_stride /* 0 or L*N */, int n_terms, const uint64_t *d_addend, uint64_t *d_out,
                                   int size, size_t count);
/* BFV only: abc_hip_diag_matvec_bsgs for BFV ciphertexts (Evaluator::rotate_rows :55,:60, multiply_plain :159,:196, add :92,:114):
 *   d_out = sum over j of rotate( sum over i of D[j * n_baby + i] * rotate(d_in, h_baby[i]),  h_giant[j] ),  [count][2][L][N].
 * Row (j, i) of D starts at d_diags_ntt + (j * n_baby + i) * diag_stride, diag_stride >= L * N, in NTT form
 * (abc_hip_bfv_plain_to_ntt); one set for the batch.  THE CALLER SUPPLIES ROWS ALREADY ROTATED BY -h_giant[j]: encode the
 * cleartext diagonal of step h_giant[j] + h_baby[i] with each half-row rolled by -h_giant[j], so no plaintext-rotation entry is
 * needed.  Sequence: the baby rotations as abc_hip_rotate runs them, into an arena; ONE in-place forward transform of all baby
 * slabs (step 0 gets a transformed copy: d_in stays untouched); per giant step one abc_hip_bfv_multiply_plain_sum with
 * ABC_HIP_CT_NTT terms -- no forward transform -- into a second arena; then d_out = d_out + rotate(inner_j, h_giant[j]) as
 * abc_hip_rotate_add does, fused where its route says so.  Bit-identical to that sequence of calls.  Order, duplicates, groups,
 * empty lists and count == 0 as in abc_hip_diag_matvec_bsgs.  Every step and every key is checked before the first launch; a CKKS
 * context, a bad stride, a negative count, a null step list, a null d_in, d_out or d_diags_ntt, a step without a key (or a NAF chain of keys), d_out overlapping d_in
 * or d_diags_ntt fail the call with nothing written.  Route: ABC_HIP_ROUTE_BFV_MATVEC_BSGS.  Capturable like abc_hip_rotate_add. */
int abc_hip_bfv_diag_matvec_bsgs(abc_hip_ctx *ctx, const uint64_t *d_in, const uint64_t *d_diags_ntt, size_t diag_stride /* >= L*N */,
                                 const int *h_baby, int n_baby, const int *h_giant, int n_giant, uint64_t *d_out, size_t count);
/* The three plaintext operations.  d_out may be d_ct (the reference's *_inplace call sites); size = 2 or 3.
 * plain_stride, in words, is the distance from ciphertext i's plaintext to ciphertext i + 1's:
 *   0            one plaintext, broadcast to the batch (d_plain holds N words for BFV, nl * N for CKKS);
 *   BFV:  N      one plaintext per ciphertext, d_plain [count][N];
 *   CKKS: >= nl * N  one plaintext per ciphertext; row i starts at d_plain + i * plain_stride and its first nl limbs are read.
 *                A stride above nl * N is how plaintexts laid out for a higher level ([count][L][N], stride L * N) are
 *                applied to ciphertexts at nl < L: limb j is modulo q_j at every level.
 * Any other stride would read past a row or let rows overlap: the call fails (non-zero status) and enqueues nothing. */
/* Evaluator::multiply_plain(_inplace) (:159,:196) */
int abc_hip_multiply_plain(abc_hip_ctx *ctx, const uint64_t *d_ct, const uint64_t *d_plain, size_t plain_stride,
                           uint64_t *d_out, int size, int nl, size_t count);
/* Evaluator::add_plain(_inplace) (:134,:175) */
int abc_hip_add_plain(abc_hip_ctx *ctx, const uint64_t *d_ct, const uint64_t *d_plain, size_t plain_stride, uint64_t *d_out,
                      int size, int nl, size_t count);
/* Evaluator::sub_plain(_inplace) (:145,:184) */
int abc_hip_sub_plain(abc_hip_ctx *ctx, const uint64_t *d_ct, const uint64_t *d_plain, size_t plain_stride, uint64_t *d_out,
                      int size, int nl, size_t count);
/* CKKS only: Evaluator::rescale_to_next / mod_switch_to_next (no reference call site).
 * d_in [count][size][nl][N] -> d_out [count][size][nl-1][N]; d_out must not alias d_in (error otherwise). */
int abc_hip_rescale(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int size, int nl, size_t count);
int abc_hip_mod_switch(abc_hip_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int size, int nl, size_t count);
/* CKKS only: Evaluator::multiply_plain and rescale_to_next as one call, the weight step of a linear layer.
 * d_ct [count][size][nl][N] -> d_out [count][size][nl-1][N], size = 2 or 3; d_plain and plain_stride exactly as
 * abc_hip_multiply_plain takes them (0: one plaintext for the batch; >= nl * N: one per ciphertext, its first nl limbs read, so
 * rows encoded at a higher level apply at a lower one).  Bit-identical to abc_hip_multiply_plain into a temporary followed by
 * abc_hip_rescale.  Where the route allows it (abc_hip_route, ABC_HIP_ROUTE_MULTIPLY_PLAIN_RESCALE: the LDS-resident rescale of
 * the rings 2^10 .. 2^14) the product is formed in the loads of the two rescale kernels and never reaches memory; otherwise the
 * product lands in an arena and the rescale runs on it.  Fails with nothing written or enqueued for a BFV context, nl < 2 or a
 * bad level, a bad stride, a size other than 2 or 3, and d_out overlapping d_ct or d_plain.  count == 0 succeeds and enqueues
 * nothing.  Capturable, under the "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_multiply_plain_rescale(abc_hip_ctx *ctx, const uint64_t *d_ct, const uint64_t *d_plain, size_t plain_stride,
                                   uint64_t *d_out, int size, int nl, size_t count);

/* ---- CKKS: scalar constants and polynomial evaluation (an activation behind a linear layer) ----
 * In NTT form the constant c at scale s is the plaintext whose every word of limb j is round(c * s) mod q_j: a scalar operand is one
 * word per limb, and needs neither an encode (an N/2-point transform and nl NTTs) nor a plaintext of nl * N equal-per-limb words
 * in memory.  The words: r = value * scale rounded to the nearest integer, ties away from zero; h_words[j] = r mod q_j in [0, q_j)
 * (a negative r maps to q_j - (|r| mod q_j), 0 stays 0).  Fails, with h_words untouched, for a BFV context, a bad nl, a non-finite
 * product or |r| >= 2^62 (the encoder's own limit).  No GPU work.  For a dyadic value * scale these are the words of
 * abc_hip_ckks_encode on N/2 copies of the value; the encoder's fp64 transform may round coefficient 0 of another constant one
 * unit away. */
int abc_hip_ckks_const_words(abc_hip_ctx *ctx, double value, double scale, int nl, uint64_t *h_words);
/* A scalar-weighted sum of ciphertexts, each term read at ITS OWN level:
 *   d_out [count][size][nl][N] = (d_addend or 0) + const (component 0 only) + w_0 * ct_0 + ... + w_{K-1} * ct_{K-1},  size = 2 or 3.
 * h_ct: HOST array of n_terms device pointers; ct_k is [count][size][h_ct_nl[k]][N] with h_ct_nl[k] >= nl (h_ct_nl == NULL: every
 * term at nl) and its first nl limbs are read in place -- abc_hip_mod_switch down to nl without the copy.  h_weights [n_terms][nl]
 * and h_const [nl] (or NULL) are HOST words as abc_hip_ckks_const_words makes them, each below its prime; everything is read
 * during the call only, and the words travel by value in the kernel arguments, eight terms per launch, the running sum carried by
 * pointer from launch to launch.  One pointer may appear in several terms; d_out may be exactly d_addend.  Bit-identical to, in
 * order: abc_hip_mod_switch repeated down to nl, abc_hip_multiply_plain per term with the constant plaintext, abc_hip_add,
 * abc_hip_add_plain for the constant.  ABC_HIP_NO_CONST_MAC_SUM=1 runs that sequence on plaintexts filled in an arena instead of
 * the K-term kernel.  n_terms == 0 writes the addend plus the constant, or the constant over zeros; count == 0 succeeds and
 * enqueues nothing.  Fails with nothing written or enqueued for: a BFV context, a bad level or size, h_ct_nl[k] < nl or > L,
 * n_terms < 0, a null term pointer, a weight or constant word >= q_j, d_out overlapping any term, d_out overlapping d_addend
 * without being equal to it.  Capturable, under the "run once eagerly first" rule of abc_hip_graph_begin. */
int abc_hip_multiply_const_sum(abc_hip_ctx *ctx, const uint64_t *const *h_ct, const int *h_ct_nl, const uint64_t *h_weights, int n_terms,
                               const uint64_t *h_const, const uint64_t *d_addend, uint64_t *d_out, int size, int nl, size_t count);
/* nl >= 2: the same sum with ONE rescale behind it, d_out [count][size][nl-1][N].  Bit-identical to abc_hip_multiply_const_sum into
 * a temporary followed by abc_hip_rescale; n_terms == 1 without addend and constant gives the words of
 * abc_hip_multiply_plain_rescale with the constant plaintext.  Route (abc_hip_route, ABC_HIP_ROUTE_CONST_SUM_RESCALE): the
 * rescale's route, then constsum=fused -- K-term forms of the two LDS-resident rescale kernels with the scalar weight in place of a
 * loaded plaintext word form the sum in their loads, so it never reaches memory -- or constsum=separate -- the sum into a context
 * arena, then the rescale.  The fused pair takes 1 .. 4 terms that all sit at level nl, on rings 2^10 .. 2^14; never N >= 2^15,
 * ABC_HIP_NO_FUSED=1, ABC_HIP_NO_ISPLIT=1 on a chain with a prime above 2^50, ABC_HIP_NO_CONST_MAC_SUM=1, more than four terms, or a
 * term above nl.  Within that it is the default where the measurement has it faster (at least 64 polynomials, count * size, and
 * 2^20 coefficients among them); ABC_HIP_CONST_SUM_RESCALE_FUSED=1 / =0 force it on and off.  Refusals as above, and nl < 2, and
 * d_out overlapping d_addend at all (the shapes differ). */
int abc_hip_multiply_const_sum_rescale(abc_hip_ctx *ctx, const uint64_t *const *h_ct, const int *h_ct_nl, const uint64_t *h_weights,
                                       int n_terms, const uint64_t *h_const, const uint64_t *d_addend, uint64_t *d_out, int size, int nl,
                                       size_t count);
/* Levels p(x) of degree `degree` consumes: ceil(log2 degree) + 1; -1 for degree < 1. */
int abc_hip_ckks_poly_eval_depth(int degree);
/* p(x) = c_0 + c_1 x + ... + c_d x^d on d_x [count][2][nl][N] at scale x_scale; h_coeffs [degree + 1], c_0 first;
 * d_out [count][2][nl - depth][N] at scale out_scale.  The sequence is FIXED (tests/poly_eval_spec.py restates it on the oracle):
 *   x^1 = x: level(1) = nl, scale(1) = x_scale.  For k = 2 .. d: e = ceil(log2 k), h = 2^(e-1), l = k - h,
 *   x^k = rescale( mul_relin( x^h, mod_switch(x^l down to nl - e + 1 limbs) ) ), level(k) = nl - e,
 *   scale(k) = scale(h) * scale(l) / q_{nl-e}, tracked in doubles on the host (a power of two is a square).
 *   A power that no non-zero coefficient and no later power needs is skipped, and a term with a zero coefficient is left out of
 *   the sum: no output word changes.
 *   E = ceil(log2 d) (0 for d = 1), m = nl - E;  W_k = const_words(c_k, out_scale * q_{m-1} / scale(k), m),
 *   W_0 = const_words(c_0, out_scale * q_{m-1}, m);  the output is ONE abc_hip_multiply_const_sum_rescale at level m over
 *   k = 1 .. d with h_ct_nl[k] = level(k): every term lands at out_scale after the one rescale, at level m - 1.
 * abc_hip_ckks_const_words holds every weight below 2^62; the constant term enters at out_scale * q_{m-1}, so
 * |c_0| * out_scale * q_{m-1} < 2^62 is required: 30-bit rescaling primes at scale 2^30, or a smaller out_scale on wider ones.
 * The powers live in a context arena; the batch is walked in groups of ciphertexts that keep THAT arena within 4 GiB (the rule of
 * abc_hip_mul_sum_relin; with ABC_HIP_CHUNK=c exactly c * lanes); three more arenas hold one ciphertext per member of the group
 * each: the lowered factor, the product before its rescale, and the last step's sum.  count == 0 succeeds and enqueues nothing.  Fails with nothing
 * written for: a BFV context, degree < 1 or > 31, nl < E + 2, a non-finite or non-positive scale, a non-finite coefficient, a
 * weight past 2^62, no relinearisation key, d_out overlapping d_x.  Route (ABC_HIP_ROUTE_POLY_EVAL): the abc_hip_mul_relin route at
 * nl, then constsum=separate -- for degree 2 and above, whose last step reads powers held above its level; at degree 1 the one term
 * sits at nl and the last step follows ABC_HIP_ROUTE_CONST_SUM_RESCALE at nl (fused from 64 polynomials on).  Capturable under the run-once rule; the recorded kernels hold the weights by value.
 * NOT in it: Paterson-Stockmeyer; folding the coefficients into the last multiplication to save the extra level; Chebyshev
 * bases; products batched across powers or through abc_hip_mul_sum_relin. */
int abc_hip_ckks_poly_eval(abc_hip_ctx *ctx, const uint64_t *d_x, double x_scale, const double *h_coeffs, int degree, double out_scale,
                           uint64_t *d_out, int nl, size_t count);

/* ---- HIP-graph capture of an operation sequence (a recorded circuit in place of the
 * eager per-call dispatch of SpecialRuntimeVisitor, src/runtime/RuntimeVisitor.cpp:40-159).
 * Everything enqueued on the context between begin and end is recorded instead of executed; the sequence must have
 * run once eagerly before (so that no scratch allocation happens while capturing) and may only use device pointers
 * that stay valid for every launch.  abc_hip_encrypt* / abc_hip_keygen* / abc_hip_keyed_* / *_h2d / *_d2h are not capturable.
 * Buffers: abc_hip_malloc inside a capture is served from the cache only (never the driver).  Every buffer the recorded
 * sequence can have touched is pinned to the graph until abc_hip_graph_destroy: the blocks the capture itself allocated or
 * freed, and EVERY abc_hip_malloc block of this context that is still out with the caller when abc_hip_graph_end runs (so an
 * operand that existed before the capture and is freed only after it -- a cached plaintext, an input -- is covered too).
 * Freeing a pinned block parks it instead of recycling it, so a replay can never run over memory that has been handed to
 * someone else; a block pinned by several graphs returns to the cache when the last of them is destroyed.  Memory that did not
 * come from abc_hip_malloc is the caller's to keep alive.  A buffer that existed before the capture
 * and is freed inside it is an INPUT of the circuit: it keeps its address and contents are the caller's to refresh before a
 * replay (HipCiphertextFactory::rewriteCiphertext).
 * Context state: scratch arenas, keys and key mirrors (fp64 twins, Shoup quotients) outlive every graph that may have recorded
 * them.  An eager call after abc_hip_graph_end may grow an arena: the old one is held back until the last graph that may read it
 * is destroyed (abc_hip_ctx_info 6 counts what is held).  A replay uses the keys that are current when it is LAUNCHED:
 * abc_hip_load_*_key and abc_hip_keygen wait for enqueued work, then rewrite each key and its mirrors in place; a Galois key
 * that keygen drops (an element outside the default set) is held back like an arena. */
int abc_hip_graph_begin(abc_hip_ctx *ctx);
int abc_hip_graph_end(abc_hip_ctx *ctx, void **graph_exec_out);
int abc_hip_graph_launch(abc_hip_ctx *ctx, void *graph_exec);
int abc_hip_graph_destroy(abc_hip_ctx *ctx, void *graph_exec);

/* ---- raw transforms, exposed for kernel-level parity tests and profiling ---- */
/* mod_kind: 0 = key-level prime `index`, 1 = BEHZ Bsk prime `index`, 2 = plaintext modulus */
int abc_hip_ntt_forward(abc_hip_ctx *ctx, uint64_t *d_data, int mod_kind, int index, size_t count);
int abc_hip_ntt_inverse(abc_hip_ctx *ctx, uint64_t *d_data, int mod_kind, int index, size_t count);
/* forward / inverse transform of whole polynomials at a data level: d_data [polys][nl][N], limb j modulo q_j
 * (CKKS plaintexts and ciphertexts travel in NTT form; host-side encoders produce coefficient form) */
int abc_hip_ntt_limbs(abc_hip_ctx *ctx, uint64_t *d_data, int nl, size_t polys, int inverse);
/* key-switch contribution only: d_target [count][nl][N] -> d_out2 [count][2][nl][N]; key_kind 0 relin, else Galois elt */
int abc_hip_keyswitch(abc_hip_ctx *ctx, const uint64_t *d_target, uint32_t key_kind, uint64_t *d_out2, int nl, size_t count);
/* micro-benchmarks of the integer / fp64 pipes (returns elapsed ms for `iters` dependent modmuls per lane); probe kernels,
 * present only in a library built with -DABC_HIP_WITH_MICROBENCH (python -m abc_amd.build --microbench), an error otherwise */
int abc_hip_microbench(abc_hip_ctx *ctx, int which, int iters, double *ms_out);
/* elapsed milliseconds between two HIP events recorded on the context stream */
int abc_hip_timer_start(abc_hip_ctx *ctx);
int abc_hip_timer_stop(abc_hip_ctx *ctx, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif
