// The CKKS slot codec of HipCiphertextFactory on the device (abc_hip_ckks_encode / _decode, the default) against its host twin
// (CkksEncoder.hpp, HipSchemeConfig::hostCkksCodec = true): two factories with the same seed run the same work, and the
// decoded values must agree with the inputs and with each other.  Prints the wall time of encryption and decryption on both.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <random>

#include "../../include/abc_hip.h"
#include "CircuitRuntime.hpp"
#include "CkksEncoder.hpp"
#include "HipCiphertext.hpp"
#include "HipCiphertextFactory.hpp"
#include "mini_test.hpp"

static void expectClose(const std::vector<double> &got, const std::vector<double> &want, double tol, const std::string &what) {
  if (got.size() < want.size()) throw std::runtime_error(what + ": too few values");
  for (size_t i = 0; i < want.size(); ++i)
    if (!(std::fabs(got[i] - want[i]) <= tol * std::fmax(1.0, std::fabs(want[i]))))
      throw std::runtime_error(what + ": slot " + std::to_string(i) + " got " + std::to_string(got[i]) + " want " + std::to_string(want[i]));
}

static HipSchemeConfig config(bool host, size_t batch) {
  HipSchemeConfig cfg;
  cfg.ckks = true;
  cfg.ringDegree = 16384;
  cfg.seed = 0xC0DEC5EEDull;
  cfg.batch = batch;
  cfg.hostCkksCodec = host;
  return cfg;
}
static const char *tag(bool host) { return host ? " [host codec]" : " [device codec]"; }

int main() {
  MiniTest t;
  const size_t slots = 8192;
  std::mt19937_64 rng(17);
  std::uniform_real_distribution<double> dist(-1.0, 1.0);
  std::vector<double> x(slots), w(slots);
  for (auto &v : x) v = dist(rng);
  for (auto &v : w) v = dist(rng);

  for (bool host : {false, true}) {
    HipCiphertextFactory f(config(host, 1));
    t.run((std::string("createCiphertext -> decryptCiphertextReal") + tag(host)).c_str(), [&] {
      auto a = f.createCiphertext(x);
      std::vector<double> got;
      f.decryptCiphertextReal(*a, got);
      EXPECT_TRUE(got.size() == slots);
      expectClose(got, x, 1e-6, "decrypt");
      auto s = f.createCiphertext(std::vector<double>{0.25, -3.5});  // padded with its last value
      f.decryptCiphertextReal(*s, got);
      std::vector<double> want(slots, -3.5);
      want[0] = 0.25;
      expectClose(got, want, 1e-6, "short input");
    });
    t.run((std::string("multiplyPlain operand decodes to its values") + tag(host)).c_str(), [&] {
      auto a = f.createCiphertext(x);
      auto m = a->multiplyPlain(Cleartext<double>(w));
      std::vector<double> got, want(slots);
      for (size_t i = 0; i < slots; ++i) want[i] = x[i] * w[i];
      f.decryptCiphertextReal(*m, got);
      expectClose(got, want, 1e-5, "multiplyPlain");
      // the operand multiplyPlain used (level 4, default scale): cached, so this returns the same device plaintext
      const int level = f.dataLimbs();
      const uint64_t *d = f.cachedCkksPlaintext(w, level, f.defaultScale());
      const size_t words = (size_t)level * f.getCiphertextSlotSize();
      void *tmp = nullptr;
      abcHipCheck(abc_hip_malloc(f.context(), &tmp, words * 8), "alloc");
      abcHipCheck(abc_hip_memcpy_d2d(f.context(), tmp, d, words * 8), "copy");
      abcHipCheck(abc_hip_ntt_limbs(f.context(), static_cast<uint64_t *>(tmp), level, 1, 1), "inverse NTT");
      std::vector<uint64_t> coeffs(words);
      abcHipCheck(abc_hip_memcpy_d2h(f.context(), coeffs.data(), tmp, words * 8), "download");
      abc_hip_free(f.context(), tmp);
      std::vector<uint64_t> primes;
      for (int j = 0; j < level; ++j) primes.push_back(f.prime(j));
      CkksEncoder enc(f.getCiphertextSlotSize(), primes);
      std::vector<double> dec;
      enc.decode(coeffs.data(), level, f.defaultScale(), dec);
      expectClose(dec, w, 1e-7, "plain operand");
    });
  }

  // config 3 shape through the interpreter, batch mode: dot product of two length-8192 vectors, B = 4 instances
  const size_t B = 4;
  std::vector<std::vector<double>> xs(B, std::vector<double>(slots)), ys(xs);
  for (auto &r : xs)
    for (auto &v : r) v = dist(rng);
  for (auto &r : ys)
    for (auto &v : r) v = dist(rng);
  std::vector<std::vector<double>> results[2];
  for (bool host : {false, true}) {
    t.run((std::string("config 3 circuit through CircuitRuntime, batch mode") + tag(host)).c_str(), [&] {
      HipCiphertextFactory f(config(host, B));
      // warm-up: tables, workspace, kernels
      std::vector<double> warm;
      f.decryptCiphertextReal(*f.createCiphertext(x), warm);
      f.queueBatchedRealInput(xs);
      f.queueBatchedRealInput(ys);
      using clk = std::chrono::steady_clock;
      const auto t0 = clk::now();
      CircuitRuntime rt(f, "secret int __input0__ = {0}; secret int __input1__ = {0};");
      f.synchronize();
      const auto t1 = clk::now();
      std::string prog = "secret int r = __input0__ *** __input1__;\n";
      for (int step = 4096; step >= 1; step /= 2) prog += "r = r +++ rotate(r, " + std::to_string(step) + ");\n";
      rt.executeAst(prog);
      auto out = rt.getOutput("y = r;");
      auto &res = *dynamic_cast<AbstractCiphertext *>(out[0].second.get());
      f.synchronize();
      const auto t2 = clk::now();
      std::vector<std::vector<double>> dec;
      f.decryptCiphertextRealBatch(res, dec);
      const auto t3 = clk::now();
      auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
      std::printf("  timing%s B=%zu: encrypt %.3f ms, compute %.3f ms, decrypt %.3f ms\n", tag(host), B, ms(t0, t1), ms(t1, t2),
                  ms(t2, t3));
      EXPECT_TRUE(dec.size() == B);
      for (size_t b = 0; b < B; ++b) {
        double dot = 0;
        for (size_t i = 0; i < slots; ++i) dot += xs[b][i] * ys[b][i];
        for (size_t i = 0; i < slots; i += 511)
          if (std::fabs(dec[b][i] - dot) > 1e-4 * std::fmax(1.0, std::fabs(dot)))
            throw std::runtime_error("instance " + std::to_string(b) + " slot " + std::to_string(i) + ": got " + std::to_string(dec[b][i]) +
                                     " want " + std::to_string(dot));
      }
      results[host ? 1 : 0] = dec;
    });
  }
  t.run("device and host codec give the same decoded circuit results", [&] {
    EXPECT_TRUE(results[0].size() == B && results[1].size() == B);
    for (size_t b = 0; b < B; ++b) expectClose(results[0][b], results[1][b], 1e-6, "instance " + std::to_string(b));
  });
  return t.summary();
}
