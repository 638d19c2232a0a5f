// HipCiphertextFactory -- AbstractCiphertextFactory over libabc_hip.so.  Drop-in counterpart of
// SealCiphertextFactory (include/ast_opt/runtime/SealCiphertextFactory.h:13-120,
// src/runtime/SealCiphertextFactory.cpp): BFV, N = numElementsPerCiphertextSlot (default 16384, :16),
// coefficient modulus BFVDefault(N) (:80), plaintext modulus Batching(N, 20) (:83), secret / public /
// relinearisation / all default Galois keys (:89-93), pad-with-last-value (:102-115).
#pragma once

#include <deque>
#include <memory>
#include <iosfwd>
#include <string>
#include <vector>

#include "CkksEncoder.hpp"
#include "GraphCapable.hpp"
#include "plugin_api.hpp"

struct abc_hip_ctx;

// Scheme policy of a HipCiphertextFactory.  The default is the reference's own choice (BFV, BFVDefault(N), Batching(N, 20):
// SealCiphertextFactory.cpp:72-100).  CKKS is the hook the reference left open (CMakeLists.txt:216, HAVE_SEAL_CKKS): a
// modulus chain given by bit sizes (data limbs, then the special prime) and a default scale.  The caller of the plugin
// surface needs nothing else: levels and scales are tracked per ciphertext, ct x ct and ct x plain products are rescaled
// (one limb dropped) while limbs remain, and operands at different levels are brought to the lower one.
struct HipSchemeConfig {
  bool ckks = false;
  unsigned int ringDegree = 16'384;
  std::vector<int> ckksBits = {50, 40, 40, 40, 50};  // the benchmark chain
  double ckksScale = 1099511627776.0;                // 2^40
  int device = 0;
  uint64_t seed = 0;  // 0: keys and encryption randomness from the OS-keyed generator; else the reproducible TEST spec
  size_t batch = 1;
  // CKKS slot codec on the host (CkksEncoder.hpp) instead of the device (abc_hip_ckks_encode / _decode): for A/B runs
  bool hostCkksCodec = false;
  // `lhs +++ rotate(v, k)` as one abc_hip_rotate_add (HipCiphertext::addRotatedInplace); off: rotateRows + addInplace, for A/B
  // runs and so that a test can compare both paths in one process
  bool fuseRotateAdd = true;
  // CKKS `ct * weights` as one abc_hip_multiply_plain_rescale (HipCiphertext::multiplyPlainInplace at two limbs or more); off:
  // abc_hip_multiply_plain, then abc_hip_rescale.  The words are the same either way, so it stays on; off is for A/B runs and tests
  bool fuseMultiplyPlainRescale = true;
  // `x *** y +++ u *** v (+++ ...)` as ONE abc_hip_mul_sum_relin (HipCiphertext::mulSum; CircuitRuntime recognises the run): the sum
  // of the size-3 products is relinearised once.  OFF by default: the result decrypts to the same values, with one key switch's
  // noise instead of one per product, but its words are not those of the per-product sequence
  bool lazyRelinearize = false;
  // BFV `x *** p +++ y *** q (+++ ...)` as ONE abc_hip_bfv_multiply_plain_sum (HipCiphertext::plainSum; CircuitRuntime recognises the
  // run): one inverse transform for the sum, public values transformed once and cached.  The words are those of multiplyPlain per
  // product and addInplace, so it stays on; off is for A/B runs and tests.  CKKS fuses only with lazyRescale below (multiplyPlain
  // rescales per product)
  // Recorded circuits: a recording holds the device pointers of the cached plaintexts it was recorded with (up to 32 per plainSum
  // node; plainCache's single pointers likewise).  Public values used between compile and the last replay must not push those out of
  // the 32-entry caches: a program that cycles through more distinct public values than that replays recordings before it does
  bool fusePlainSum = true;
  // CKKS `x *** p +++ y *** q (+++ ...)` as ONE abc_hip_multiply_plain_sum_rescale (HipCiphertext::plainSum; needs fusePlainSum): the
  // sum of the products is rescaled once.  OFF by default, like lazyRelinearize: the result decrypts to the same values, with one
  // rescale rounding instead of one per product, but its words are not those of multiplyPlain per product and addInplace
  bool lazyRescale = false;
  // CKKS plain operations whose public value is ONE number (every entry equal: `x *** 0.5`, `x +++ 3`, `x --- 0.25`) take the scalar as
  // per-limb words in the kernel arguments (abc_hip_ckks_const_words, abc_hip_multiply_const_sum_rescale / abc_hip_multiply_const_sum):
  // no vector is expanded, nothing is encoded, no plaintext is cached.  OFF by default, like lazyRescale: the device encoder's fp64
  // transform may round coefficient 0 of a non-dyadic constant one unit away from const_words, so the ciphertext words are not
  // guaranteed to be those of the encoded path (they are for dyadic values); the decoded values agree within the CKKS tolerance
  bool constOperands = false;
};

class HipCiphertextFactory : public AbstractCiphertextFactory, public GraphCapable {
  const unsigned int ciphertextSlotSize = 16'384;
  abc_hip_ctx *ctx = nullptr;  // owned: device tables + keys
  int limbs = 0;               // data limbs L
  uint64_t keySeed = 0;
  // Batch mode (an extension the reference lacks; it evaluates one circuit at a time, RuntimeVisitor.h:34): every
  // ciphertext of this factory is B independent ciphertexts that all operations process in one batched device call, so
  // ONE pass of an unchanged interpreter (ABC's RuntimeVisitor or CircuitRuntime) evaluates the circuit on B input sets.
  size_t batch = 1;
  mutable std::deque<std::vector<std::vector<int64_t>>> queuedInputs;
  mutable std::deque<std::vector<std::vector<double>>> queuedRealInputs;
  // Encoded plaintexts of recent plain operands (the reference re-encodes its operand on every plain operation,
  // SealCiphertext.cpp:132,143,154: here a repeated constant costs one encode + upload, and no device synchronisation)
  struct CachedPlain {
    std::vector<int64_t> values;
    uint64_t *d_plain;
  };
  mutable std::deque<CachedPlain> plainCache;
  static constexpr size_t kPlainCacheEntries = 32;
  // The same operands lifted and in NTT form, [L][N] (abc_hip_bfv_plain_to_ntt), least recently used first.  An entry's block is
  // shared with whoever asked for it: HipCiphertext::plainSum gathers up to kPlainCacheEntries of them before its one call, and an
  // eviction by a later miss of the same gathering must not free a block gathered earlier -- the block goes when its last holder does
 public:
  struct DeviceBlock {
    abc_hip_ctx *ctx;
    uint64_t *p;
    DeviceBlock(abc_hip_ctx *c, uint64_t *ptr) : ctx(c), p(ptr) {}
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock();  // abc_hip_free: stream-ordered, so every call enqueued before this point has its operand
  };

 private:
  struct CachedNttPlain {
    std::vector<int64_t> values;
    std::shared_ptr<const DeviceBlock> block;
  };
  mutable std::deque<CachedNttPlain> plainNttCache;

  // CKKS policy (empty / unused for BFV)
  bool ckksMode = false;
  double ckksScale = 0;
  double ckksScaleTol = 0;  // relative scale difference additions accept (setupContext: from the chain)
  std::vector<int> ckksBits;
  std::vector<uint64_t> chain;  // the context's primes: data limbs, then the special prime
  uint64_t plainModulus = 0;    // BFV t (0 for CKKS)
  CkksEncoder ckksEncoder;    // host twin of the device codec (HipSchemeConfig::hostCkksCodec)
  bool hostCkksCodec = false;
  bool fuseRotateAdd = true;
  mutable size_t fusedRotateAdds = 0;  // abc_hip_rotate_add calls issued by addRotatedInplace
  bool fuseMultiplyPlainRescale = true;
  mutable size_t fusedMultiplyPlainRescales = 0;  // abc_hip_multiply_plain_rescale calls issued by multiplyPlainInplace
  bool lazyRelin = false;
  mutable size_t lazyMulSums = 0;  // abc_hip_mul_sum_relin calls issued by HipCiphertext::mulSum
  bool fusePlainSums = true;
  mutable size_t plainSums = 0;  // abc_hip_bfv_multiply_plain_sum calls issued by HipCiphertext::plainSum
  bool lazyRescale = false;
  mutable size_t plainSumRescales = 0;  // abc_hip_multiply_plain_sum_rescale calls issued by HipCiphertext::plainSum
  bool constOperands = false;
  mutable size_t constOperandOps = 0;  // abc_hip_multiply_const_sum(_rescale) calls issued by the three plain operations of HipCiphertext
  // oldest first; the block is shared with a caller that holds it (cachedCkksPlaintextBlock), as in plainNttCache
  struct CachedCkksPlain {
    std::vector<double> values;
    int level;
    double scale;
    std::shared_ptr<const DeviceBlock> block;
  };
  mutable std::deque<CachedCkksPlain> ckksPlainCache;

  void setupContext(int device);
  template <typename T>
  std::vector<T> expandVector(const std::vector<T> &values) const;
  std::unique_ptr<AbstractCiphertext> createCkksCiphertext(const std::vector<double> &data) const;
  // rows [count][N/2] of slot values -> device plaintexts [count][level][N] (NTT form); caller frees
  uint64_t *encodeCkks(const std::vector<double> &rows, size_t count, int level, double scale) const;
  int encryptInto(const void *d_plain, uint64_t *d_ct) const;

 public:
  HipCiphertextFactory();
  explicit HipCiphertextFactory(unsigned int numElementsPerCiphertextSlot, int device = 0, uint64_t seed = 0, size_t batchSize = 1);
  explicit HipCiphertextFactory(const HipSchemeConfig &config);
  virtual ~HipCiphertextFactory();  // (ABC's AbstractCiphertextFactory declares no virtual destructor)
  HipCiphertextFactory(const HipCiphertextFactory &) = delete;  // one device context per factory
  HipCiphertextFactory &operator=(const HipCiphertextFactory &) = delete;

  [[nodiscard]] abc_hip_ctx *context() const { return ctx; }
  [[nodiscard]] unsigned int getCiphertextSlotSize() const { return ciphertextSlotSize; }
  [[nodiscard]] int dataLimbs() const { return limbs; }
  [[nodiscard]] size_t batchSize() const { return batch; }
  [[nodiscard]] size_t ciphertextWords() const { return batch * 2 * limbs * ciphertextSlotSize; }  // of one (batched) value
  [[nodiscard]] size_t ciphertextWords(int level) const { return batch * 2 * (size_t)level * ciphertextSlotSize; }
  [[nodiscard]] bool isCkks() const { return ckksMode; }
  [[nodiscard]] bool fusesRotateAdd() const { return fuseRotateAdd; }
  void setFuseRotateAdd(bool on) { fuseRotateAdd = on; }
  [[nodiscard]] size_t fusedRotateAddCalls() const { return fusedRotateAdds; }
  void countFusedRotateAdd() const { ++fusedRotateAdds; }
  [[nodiscard]] bool fusesMultiplyPlainRescale() const { return fuseMultiplyPlainRescale; }
  void setFuseMultiplyPlainRescale(bool on) { fuseMultiplyPlainRescale = on; }
  [[nodiscard]] size_t fusedMultiplyPlainRescaleCalls() const { return fusedMultiplyPlainRescales; }
  void countFusedMultiplyPlainRescale() const { ++fusedMultiplyPlainRescales; }
  [[nodiscard]] bool lazyRelinearizes() const { return lazyRelin; }
  void setLazyRelinearize(bool on) { lazyRelin = on; }
  [[nodiscard]] size_t mulSumCalls() const { return lazyMulSums; }
  void countMulSum() const { ++lazyMulSums; }
  [[nodiscard]] bool fusesPlainSum() const { return fusePlainSums; }
  void setFusePlainSum(bool on) { fusePlainSums = on; }
  [[nodiscard]] size_t plainSumCalls() const { return plainSums; }
  void countPlainSum() const { ++plainSums; }
  [[nodiscard]] bool lazyRescales() const { return lazyRescale; }
  void setLazyRescale(bool on) { lazyRescale = on; }
  [[nodiscard]] size_t plainSumRescaleCalls() const { return plainSumRescales; }
  void countPlainSumRescale() const { ++plainSumRescales; }
  [[nodiscard]] bool takesConstOperands() const { return constOperands; }
  void setConstOperands(bool on) { constOperands = on; }
  [[nodiscard]] size_t constOperandCalls() const { return constOperandOps; }
  void countConstOperand() const { ++constOperandOps; }
  [[nodiscard]] static constexpr size_t plainCacheEntries() { return kPlainCacheEntries; }
  // BFV: device plaintext [L][N], lifted and in NTT form, of public values, from the factory's cache (least recently used out
  // first).  The block lives as long as the cache or the caller holds it: hold it until the call that reads it has been enqueued
  std::shared_ptr<const DeviceBlock> cachedPlaintextNtt(const std::vector<int> &value) const;
  [[nodiscard]] double defaultScale() const { return ckksScale; }
  // CKKS: largest relative difference between the scales of two addends that is drift, not a mismatch
  [[nodiscard]] double scaleTolerance() const { return ckksScaleTol; }
  [[nodiscard]] uint64_t prime(int j) const { return chain[j]; }
  // slots a value may fill: N for BFV (two rows of N/2), N/2 for CKKS (one row; rotateRows rotates it cyclically)
  [[nodiscard]] unsigned int usableSlots() const { return ckksMode ? ciphertextSlotSize / 2 : ciphertextSlotSize; }
  // CKKS: device plaintext [level][N] (NTT form) of public values at a given level and scale, from the factory's cache: valid until
  // kPlainCacheEntries further distinct operands have been encoded (the oldest entry goes on a miss; release is stream-ordered)
  const uint64_t *cachedCkksPlaintext(const std::vector<double> &value, int level, double scale) const;
  // the same entry as a shared block, for a caller that gathers several before one call (HipCiphertext::plainSum): a later miss of
  // the same gathering may push the entry out of the cache, the block lives until its last holder lets go
  std::shared_ptr<const DeviceBlock> cachedCkksPlaintextBlock(const std::vector<double> &value, int level, double scale) const;
  // CKKS: all slot values of instance 0 as doubles (decryptCiphertext rounds them to the interface's int64)
  void decryptCiphertextReal(AbstractCiphertext &abstractCiphertext, std::vector<double> &out) const;
  void decryptCiphertextRealBatch(AbstractCiphertext &abstractCiphertext, std::vector<std::vector<double>> &out) const;
  // batch mode for real-valued inputs (CKKS)
  void queueBatchedRealInput(std::vector<std::vector<double>> perInstance) const;
  std::unique_ptr<AbstractCiphertext> createCiphertext(const std::vector<double> &data) const;

  // Batch mode: the next createCiphertext call encrypts these B vectors (one per circuit instance) instead of B copies
  // of its argument; calls are served in queue order, i.e. in the order the interpreter declares its secret inputs.
  void queueBatchedInput(std::vector<std::vector<int64_t>> perInstance) const;
  // all B decrypted slot vectors of a batched ciphertext (decryptCiphertext returns instance 0, the reference's view)
  void decryptCiphertextBatch(AbstractCiphertext &abstractCiphertext, std::vector<std::vector<int64_t>> &out) const;

  // device plaintext [N] (coefficients mod t) from public values; caller frees with freeDevice
  uint64_t *createPlaintext(const std::vector<int> &value) const;
  uint64_t *createPlaintext(const std::vector<int64_t> &value) const;
  uint64_t *createPlaintext(int64_t value) const;
  void freeDevice(void *p) const;
  // same, owned by the factory's cache: valid until kPlainCacheEntries further distinct operands have been encoded
  // (release is stream-ordered, so operations already issued on an evicted plaintext stay correct)
  const uint64_t *cachedPlaintext(const std::vector<int> &value) const;

  std::unique_ptr<AbstractCiphertext> createCiphertext(const std::vector<int64_t> &data) const override;
  std::unique_ptr<AbstractCiphertext> createCiphertext(const std::vector<int> &data) const override;
  std::unique_ptr<AbstractCiphertext> createCiphertext(int64_t data) const override;
  std::unique_ptr<AbstractCiphertext> createCiphertext(std::unique_ptr<AbstractValue> &&abstractValue) const override;
  void decryptCiphertext(AbstractCiphertext &abstractCiphertext, std::vector<int64_t> &ciphertextData) const override;
  std::string getString(AbstractCiphertext &abstractCiphertext) const override;

  // ---- SEAL 3.6 wire format (SealWire.hpp: layout, provenance; PARITY UNPINNED -- no SEAL in this image) ----
  // The reference serialises nothing; this is the additive row f3 of SURVEY.md section 8: a client may keep seal::KeyGenerator /
  // Encryptor / Decryptor and hand evaluation to this backend.  compression: 0 none, 1 zlib, 2 zstd (seal::compr_mode_type).
  // A batched value is written / read as its B instances, one SEAL object after the other.
  void saveCiphertext(const AbstractCiphertext &ciphertext, std::ostream &out, int compression = 0) const;
  std::unique_ptr<AbstractCiphertext> loadCiphertext(std::istream &in) const;
  void saveSecretKey(std::ostream &out, int compression = 0) const;
  void savePublicKey(std::ostream &out, int compression = 0) const;
  void saveRelinKeys(std::ostream &out, int compression = 0) const;
  void saveGaloisKeys(std::ostream &out, int compression = 0) const;
  // replace this factory's keys by SEAL-generated ones (same parameters, checked through parms_id); seed-compressed objects
  // (Serializable<...>) are refused
  void loadSecretKey(std::istream &in);
  void loadPublicKey(std::istream &in);
  void loadRelinKeys(std::istream &in);
  void loadGaloisKeys(std::istream &in);

  // GraphCapable: recorded circuits (abc_hip_graph_*)
  void graphBegin() const override;
  void *graphEnd() const override;
  void graphAbort() const override;
  void graphLaunch(void *graph) const override;
  void graphDestroy(void *graph) const override;
  void synchronize() const override;
  void rewriteCiphertext(AbstractCiphertext &target, const std::vector<int64_t> &values) const override;
  void rewriteCiphertextBatch(AbstractCiphertext &target, const std::vector<std::vector<int64_t>> &perInstance) const override;
};

// maps a non-zero C-ABI status to the reference's error convention (std::runtime_error)
void abcHipCheck(int status, const char *what);
