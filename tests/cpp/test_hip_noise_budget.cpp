// HipCiphertext::noiseBits / noiseBitsBatch (SealCiphertext::noiseBits, src/runtime/SealCiphertext.cpp:80-83) behind the plugin
// surface: the invariant noise budget, computed on the device (abc_hip_noise_budget), against what decryption does.  Seeded
// factories, so every run sees the same keys and ciphertexts.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>

#include "../../include/abc_hip.h"
#include "HipCiphertext.hpp"
#include "HipCiphertextFactory.hpp"
#include "mini_test.hpp"

static int bitsOf(const AbstractCiphertext &c) { return dynamic_cast<const HipCiphertext &>(c).noiseBits(); }
static std::vector<int> batchBitsOf(const AbstractCiphertext &c) { return dynamic_cast<const HipCiphertext &>(c).noiseBitsBatch(); }

static std::vector<int64_t> randomSlots(std::mt19937_64 &rng, size_t n) {
  std::uniform_int_distribution<int64_t> dist(0, 1024);
  std::vector<int64_t> v(n);
  for (auto &x : v) x = dist(rng);
  return v;
}
// slot-wise product modulo t, residues in [0, t)
static void mulInto(std::vector<int64_t> &acc, const std::vector<int64_t> &v, int64_t t) {
  for (size_t i = 0; i < acc.size(); ++i) acc[i] = (int64_t)((__int128)acc[i] * v[i] % t);
}
static bool decryptsTo(HipCiphertextFactory &f, AbstractCiphertext &c, const std::vector<int64_t> &want, int64_t t) {
  std::vector<int64_t> got;
  f.decryptCiphertext(c, got);
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < want.size(); ++i)
    if (((got[i] % t) + t) % t != want[i]) return false;
  return true;
}

// multiply chain: the budget falls strictly with every product, stays positive while decryption is right and is exactly 0 from
// the depth where it is not
static void chain(unsigned n, uint64_t seed) {
  HipCiphertextFactory f(n, 0, seed);
  const int64_t t = (int64_t)abc_hip_plain_modulus_batching(n, 20);
  std::mt19937_64 rng(seed);
  std::vector<int64_t> want = randomSlots(rng, n);
  auto acc = f.createCiphertext(want);
  int bits = bitsOf(*acc);
  std::printf("  N=%u fresh: %d bits\n", n, bits);
  EXPECT_TRUE(bits > 0);
  EXPECT_TRUE(decryptsTo(f, *acc, want, t));
  bool failedOnce = false;
  for (int depth = 1; depth <= 12 && !failedOnce; ++depth) {
    const auto v = randomSlots(rng, n);
    acc->multiplyInplace(*f.createCiphertext(v));
    mulInto(want, v, t);
    const int now = bitsOf(*acc);
    const bool right = decryptsTo(f, *acc, want, t);
    std::printf("  N=%u depth %d: %d bits, decryption %s\n", n, depth, now, right ? "right" : "wrong");
    EXPECT_TRUE(now < bits);
    if (right) EXPECT_TRUE(now > 0);
    else EXPECT_TRUE(now == 0);
    failedOnce = !right;
    bits = now;
  }
  EXPECT_TRUE(failedOnce);  // the chain ran until the budget was spent
}

int main() {
  MiniTest t;
  t.run("multiply chain to budget 0, N = 4096", [] { chain(4096, 0xABC00011ull); });
  t.run("multiply chain to budget 0, N = 8192", [] { chain(8192, 0xABC00012ull); });

  t.run("rotation and addition do not raise the budget; a clone reports its source's value", [] {
    const unsigned n = 8192;
    HipCiphertextFactory f(n, 0, 0xABC00013ull);
    std::mt19937_64 rng(5);
    auto a = f.createCiphertext(randomSlots(rng, n));
    const int fresh = bitsOf(*a);
    EXPECT_TRUE(fresh > 0);
    auto c = a->clone();
    EXPECT_TRUE(bitsOf(*c) == fresh);
    a->rotateRowsInplace(3);
    const int rotated = bitsOf(*a);
    EXPECT_TRUE(rotated <= fresh && rotated > 0);
    EXPECT_TRUE(bitsOf(*c) == fresh);  // the clone kept the value the rotation replaced
    auto twin = a->clone();
    a->addInplace(*twin);  // a + a: the noise doubles
    const int added = bitsOf(*a);
    EXPECT_TRUE(added <= rotated && added > 0);
    a->addInplace(*f.createCiphertext(randomSlots(rng, n)));
    EXPECT_TRUE(bitsOf(*a) <= rotated);
    a->multiplyInplace(*c);
    const int product = bitsOf(*a);
    EXPECT_TRUE(product < added && product > 0);
    EXPECT_TRUE(bitsOf(*a->clone()) == product);
  });

  t.run("batch mode: B budgets, noiseBits is their minimum", [] {
    const unsigned n = 4096;
    const size_t B = 4;
    HipCiphertextFactory f(n, 0, 0xABC00014ull, B);
    std::mt19937_64 rng(6);
    std::vector<std::vector<int64_t>> x(B), y(B);
    for (size_t b = 0; b < B; ++b) {
      x[b] = randomSlots(rng, n);
      y[b] = randomSlots(rng, n);
    }
    f.queueBatchedInput(x);
    auto a = f.createCiphertext(std::vector<int64_t>{0});
    auto bitsA = batchBitsOf(*a);
    EXPECT_TRUE(bitsA.size() == B);
    for (int v : bitsA) EXPECT_TRUE(v > 0);
    EXPECT_TRUE(bitsOf(*a) == *std::min_element(bitsA.begin(), bitsA.end()));
    f.queueBatchedInput(y);
    a->multiplyInplace(*f.createCiphertext(std::vector<int64_t>{0}));
    auto bitsP = batchBitsOf(*a);
    EXPECT_TRUE(bitsP.size() == B);
    for (size_t b = 0; b < B; ++b) EXPECT_TRUE(bitsP[b] > 0 && bitsP[b] < bitsA[b]);
    EXPECT_TRUE(bitsOf(*a) == *std::min_element(bitsP.begin(), bitsP.end()));
    EXPECT_TRUE(batchBitsOf(*a->clone()) == bitsP);
  });

  t.run("a CKKS factory's ciphertext throws, naming the scheme", [] {
    HipSchemeConfig cfg;
    cfg.ckks = true;
    cfg.seed = 0xABC00015ull;
    HipCiphertextFactory f(cfg);
    auto a = f.createCiphertext(std::vector<double>{0.5, -1.25});
    EXPECT_THROWS(bitsOf(*a));
    EXPECT_THROWS(batchBitsOf(*a));
    std::string msg;
    try { (void)bitsOf(*a); } catch (const std::runtime_error &e) { msg = e.what(); }
    EXPECT_TRUE(msg.find("CKKS") != std::string::npos);
    std::vector<double> got;  // the factory still works
    f.decryptCiphertextReal(*a, got);
    EXPECT_TRUE(!got.empty() && std::fabs(got[0] - 0.5) < 1e-4);
  });
  return t.summary();
}
