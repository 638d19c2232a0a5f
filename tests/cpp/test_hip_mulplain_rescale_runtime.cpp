// CKKS `ct * weights` behind the plugin surface (needs a GPU): HipCiphertext::multiplyPlainInplace as one
// abc_hip_multiply_plain_rescale (HipSchemeConfig::fuseMultiplyPlainRescale, the default) against abc_hip_multiply_plain followed by
// abc_hip_rescale.  The same small program -- a weight product at two successive levels, then an add -- runs both ways on ONE factory
// from the same input ciphertext: the ciphertext words must be equal word for word, levels and scales alike, the fused-call counter
// moves only while the flag is on, and neither a product at one limb nor the -1 negation shortcut counts.  The same as a recorded
// circuit, replayed on a new input.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/abc_hip.h"
#include "CircuitRuntime.hpp"
#include "HipCiphertext.hpp"
#include "HipCiphertextFactory.hpp"
#include "mini_test.hpp"

namespace {
std::string listOf(const std::vector<int64_t> &v) {
  std::string s = "{";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "}";
}
HipCiphertext &hip(AbstractValue &v) { return dynamic_cast<HipCiphertext &>(v); }
std::vector<uint64_t> wordsOf(const HipCiphertextFactory &f, AbstractValue &v) {
  auto &c = hip(v);
  std::vector<uint64_t> w(f.ciphertextWords(c.level()));
  abcHipCheck(abc_hip_memcpy_d2h(f.context(), w.data(), static_cast<const HipCiphertext &>(c).devicePtr(), w.size() * 8), "download");
  return w;
}
AbstractValue &named(OutputIdentifierValuePairs &out, const std::string &name) {
  for (auto &p : out)
    if (p.first == name) return *p.second;
  throw std::runtime_error("no output " + name);
}

const std::vector<int64_t> W1 = {3, 1, -2, 5, 0, 7, 1, -4}, W2 = {2, -2, 1, 3, 9, 1, -1, 6};
// y1 = x (.) W1 (level 4 -> 3), y2 = y1 (.) W2 (3 -> 2), y = y2 + y2; on the copy x<sfx> of x (copy-on-write: the same input words)
std::string program(const std::string &sfx) {
  return "secret int x" + sfx + " = x;\nsecret int y1" + sfx + " = x" + sfx + " *** " + listOf(W1) + ";\nsecret int y2" + sfx + " = y1" + sfx +
         " *** " + listOf(W2) + ";\nsecret int y" + sfx + " = y2" + sfx + " +++ y2" + sfx + ";\n";
}
void sameResults(const HipCiphertextFactory &f, OutputIdentifierValuePairs &out) {
  for (const char *v : {"y1", "y2", "y"}) {
    auto &a = named(out, std::string(v) + "a"), &b = named(out, std::string(v) + "b");
    EXPECT_TRUE(hip(a).level() == hip(b).level() && hip(a).scale() == hip(b).scale());
    EXPECT_TRUE(wordsOf(f, a) == wordsOf(f, b));
  }
  EXPECT_TRUE(hip(named(out, "y1a")).level() == 3 && hip(named(out, "ya")).level() == 2);
}
void slotsAre(const HipCiphertextFactory &f, AbstractValue &y, const std::vector<int64_t> &x) {
  std::vector<double> d;
  f.decryptCiphertextReal(dynamic_cast<AbstractCiphertext &>(y), d);
  for (size_t i = 0; i < x.size(); ++i) {
    const double want = 2.0 * (double)(x[i] * W1[i] * W2[i]);
    if (!(std::fabs(d.at(i) - want) <= 1e-3)) throw std::runtime_error("slot " + std::to_string(i) + ": got " + std::to_string(d[i]) + " want " + std::to_string(want));
  }
}
const char *kOutputs = "y1a = y1a; y1b = y1b; y2a = y2a; y2b = y2b; ya = ya; yb = yb;";
}  // namespace

int main() {
  MiniTest t;
  const std::vector<int64_t> x1 = {3, 1, 4, 1, 5, 9, 2, 6}, x2 = {-7, 10, 0, 25, 8, 8, -3, 1};
  HipSchemeConfig cfg;  // the default chain {50, 40, 40, 40, 50} at N = 2^14
  cfg.ckks = true;
  cfg.seed = 0xABC0F05Eull;

  t.run("two weight products and an add, fused against separate", [&] {
    HipCiphertextFactory f(cfg);
    EXPECT_TRUE(f.fusesMultiplyPlainRescale() && f.fusedMultiplyPlainRescaleCalls() == 0);
    CircuitRuntime rt(f, "secret int x = " + listOf(x1) + ";");
    rt.executeAst(program("a"));
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 2);
    f.setFuseMultiplyPlainRescale(false);
    rt.executeAst(program("b"));
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 2);  // the separate path issues none
    auto out = rt.getOutput(kOutputs);
    sameResults(f, out);
    slotsAre(f, named(out, "ya"), x1);
    // copy-on-write: a clone taken before the product keeps the old value and level
    f.setFuseMultiplyPlainRescale(true);
    auto c = f.createCiphertext(x1);
    auto keep = c->clone();
    const auto before = wordsOf(f, *keep);
    c->multiplyPlainInplace(Cleartext<int>(std::vector<int>{2}));
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 3);
    EXPECT_TRUE(hip(*c).level() == 3 && hip(*keep).level() == 4 && wordsOf(f, *keep) == before);
    // the configuration field is what the setter sets
    HipSchemeConfig off = cfg;
    off.fuseMultiplyPlainRescale = false;
    HipCiphertextFactory g(off);
    EXPECT_TRUE(!g.fusesMultiplyPlainRescale());
    auto d = g.createCiphertext(x1);
    d->multiplyPlainInplace(Cleartext<int>(std::vector<int>{2}));
    EXPECT_TRUE(g.fusedMultiplyPlainRescaleCalls() == 0 && hip(*d).level() == 3);
  });

  t.run("one limb left, the -1 shortcut and a scale out of bounds: no fused call", [&] {
    // {50, 30, 50} at scale 2^20: a product at two limbs leaves 2^40 / q_1 ~ 2^10, which squares again under the 50 bits of one limb
    HipSchemeConfig small = cfg;
    small.ringDegree = 4096;
    small.ckksBits = {50, 30, 50};
    small.ckksScale = std::ldexp(1.0, 20);
    HipCiphertextFactory f(small);
    auto a = f.createCiphertext(x1);
    auto b = a->clone();
    const Cleartext<int> minusOne(std::vector<int>{-1}), two(std::vector<int>{2});
    a->multiplyPlainInplace(minusOne);
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 0 && hip(*a).level() == 2);  // a negation: no level is spent
    a->multiplyPlainInplace(two);
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 1 && hip(*a).level() == 1);
    const double s1 = hip(*a).scale();
    a->multiplyPlainInplace(two);  // nl == 1: the product alone, the scale stays squared
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 1 && hip(*a).level() == 1 && hip(*a).scale() == s1 * f.defaultScale());
    a->multiplyPlainInplace(minusOne);
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 1 && hip(*a).level() == 1);
    f.setFuseMultiplyPlainRescale(false);
    b->multiplyPlainInplace(minusOne);
    b->multiplyPlainInplace(two);
    b->multiplyPlainInplace(two);
    b->multiplyPlainInplace(minusOne);
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 1);
    EXPECT_TRUE(hip(*a).scale() == hip(*b).scale() && wordsOf(f, *a) == wordsOf(f, *b));
    // a scale that does not fit throws before anything is enqueued: the value keeps its words, level and scale
    f.setFuseMultiplyPlainRescale(true);
    HipSchemeConfig wide = small;
    wide.ckksScale = std::ldexp(1.0, 45);  // 2^90 against 80 bits of modulus
    HipCiphertextFactory h(wide);
    auto c = h.createCiphertext(x1);
    const auto before = wordsOf(h, *c);
    EXPECT_THROWS(c->multiplyPlainInplace(two));
    EXPECT_TRUE(h.fusedMultiplyPlainRescaleCalls() == 0 && hip(*c).level() == 2 && hip(*c).scale() == h.defaultScale());
    EXPECT_TRUE(wordsOf(h, *c) == before);
  });

  t.run("the same as a recorded circuit, replayed on a new input", [&] {
    HipCiphertextFactory f(cfg);
    CircuitRuntime rt(f, "secret int x = " + listOf(x1) + ";");
    rt.compile(program("a"));
    EXPECT_TRUE(rt.compiled());
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 4);  // compile interprets twice: eagerly, then into the recording
    for (const auto *xs : {&x1, &x2}) {
      f.setFuseMultiplyPlainRescale(true);
      if (xs == &x2) {
        rt.setInput("x", x2);
        rt.replay();
        EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 4);  // a replay dispatches nothing
      }
      f.setFuseMultiplyPlainRescale(false);
      rt.executeAst(program("b"));  // eagerly, from the same input buffer
      auto out = rt.getOutput(kOutputs);
      sameResults(f, out);
      slotsAre(f, named(out, "ya"), *xs);
    }
  });
  return t.summary();
}
