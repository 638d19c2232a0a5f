// CKKS plain operations with a public value that is ONE number, behind the plugin surface (needs a GPU): with
// HipSchemeConfig::constOperands on, HipCiphertext::multiplyPlainInplace / addPlainInplace / subtractPlainInplace take the scalar as
// per-limb words (abc_hip_ckks_const_words, abc_hip_multiply_const_sum_rescale, abc_hip_multiply_const_sum) -- no vector expanded,
// nothing encoded, no plaintext cached; off -- the default -- the encoded path.  The same small program runs both ways on ONE factory
// from the same input ciphertext.  Dyadic scalars at dyadic scales (integers on a fresh ciphertext, weights at the default scale): the
// ciphertext words are equal word for word, levels and scales alike.  Non-dyadic scalars: the encoder may round coefficient 0 one
// unit away, so the decoded values are compared, within the tolerance the plugin's CKKS tests use.  The counter moves only while the
// flag is on; the -1 negation shortcut stays ahead of it and a vector that is not one number takes the encoded path.  The same as a
// recorded circuit, replayed on a new input -- the dyadic program word for word, a program whose additions sit behind a product by values.
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
std::vector<double> slotsOf(const HipCiphertextFactory &f, AbstractValue &y) {
  std::vector<double> d;
  f.decryptCiphertextReal(dynamic_cast<AbstractCiphertext &>(y), d);
  return d;
}

// y1 = x + 2 and y2 = y1 - 5 on the fresh ciphertext (scale 2^40 exactly: 2 * 2^40 is an integer), y3 = 3 y2 (level 4 -> 3),
// y = 4 y3 (3 -> 2): weights sit at the default scale, 3 * 2^40; on the copy x<sfx> of x (copy-on-write: the same input words)
std::string program(const std::string &sfx) {
  return "secret int x" + sfx + " = x;\nsecret int y1" + sfx + " = x" + sfx + " +++ 2;\nsecret int y2" + sfx + " = y1" + sfx + " --- 5;\nsecret int y3" + sfx +
         " = y2" + sfx + " *** 3;\nsecret int y" + sfx + " = y3" + sfx + " *** 4;\n";
}
void sameResults(const HipCiphertextFactory &f, OutputIdentifierValuePairs &out) {
  for (const char *v : {"y1", "y2", "y3", "y"}) {
    auto &a = named(out, std::string(v) + "a"), &b = named(out, std::string(v) + "b");
    EXPECT_TRUE(hip(a).level() == hip(b).level() && hip(a).scale() == hip(b).scale());
    EXPECT_TRUE(wordsOf(f, a) == wordsOf(f, b));
  }
  EXPECT_TRUE(hip(named(out, "y2a")).level() == 4 && hip(named(out, "y3a")).level() == 3 && hip(named(out, "ya")).level() == 2);
}
void slotsAre(const HipCiphertextFactory &f, AbstractValue &y, const std::vector<int64_t> &x) {
  const auto d = slotsOf(f, y);
  for (size_t i = 0; i < x.size(); ++i) {
    const double want = 12.0 * (double)(x[i] - 3);
    if (!(std::fabs(d.at(i) - want) <= 1e-3)) throw std::runtime_error("slot " + std::to_string(i) + ": got " + std::to_string(d[i]) + " want " + std::to_string(want));
  }
}
const char *kOutputs = "y1a = y1a; y1b = y1b; y2a = y2a; y2b = y2b; y3a = y3a; y3b = y3b; ya = ya; yb = yb;";
}  // namespace

int main() {
  MiniTest t;
  const std::vector<int64_t> x1 = {3, 1, 4, 1, 5, 9, 2, 6}, x2 = {-7, 10, 0, 25, 8, 8, -3, 1};
  HipSchemeConfig cfg;  // the default chain {50, 40, 40, 40, 50} at N = 2^14
  cfg.ckks = true;
  cfg.seed = 0xC0257A27ull;

  t.run("dyadic scalars: the words of the encoded path, eagerly", [&] {
    HipCiphertextFactory f(cfg);
    EXPECT_TRUE(!f.takesConstOperands() && f.constOperandCalls() == 0);  // off by default
    f.setConstOperands(true);
    CircuitRuntime rt(f, "secret int x = " + listOf(x1) + ";");
    rt.executeAst(program("a"));
    EXPECT_TRUE(f.constOperandCalls() == 4);
    f.setConstOperands(false);
    rt.executeAst(program("b"));
    EXPECT_TRUE(f.constOperandCalls() == 4);  // the encoded path issues none
    auto out = rt.getOutput(kOutputs);
    sameResults(f, out);
    slotsAre(f, named(out, "ya"), x1);
    // the configuration field is what the setter sets; copy-on-write: a clone taken before keeps the old value and level
    HipSchemeConfig on = cfg;
    on.constOperands = true;
    HipCiphertextFactory g(on);
    EXPECT_TRUE(g.takesConstOperands());
    auto c = g.createCiphertext(x1);
    auto keep = c->clone();
    const auto before = wordsOf(g, *keep);
    c->multiplyPlainInplace(Cleartext<int>(std::vector<int>{2}));
    c->addPlainInplace(Cleartext<int>(std::vector<int>{1}));
    EXPECT_TRUE(g.constOperandCalls() == 2 && hip(*c).level() == 3 && hip(*keep).level() == 4 && wordsOf(g, *keep) == before);
  });

  t.run("non-dyadic scalars: the same values; -1 negates, a vector is encoded, one limb multiplies without a rescale", [&] {
    HipCiphertextFactory f(cfg);
    const Cleartext<double> w(std::vector<double>{0.3}), a(std::vector<double>{0.1}), s(std::vector<double>{1.0 / 3});
    const Cleartext<int> minusOne(std::vector<int>{-1}), vec(std::vector<int>{1, 2, 3, 4, 5, 6, 7, 8});
    auto run = [&](bool on) {
      f.setConstOperands(on);
      auto c = f.createCiphertext(x1);
      c->multiplyPlainInplace(w);     // 4 -> 3
      c->addPlainInplace(a);          // at the product's scale 2^80 / q_3: not an integer times 2^k
      c->subtractPlainInplace(s);
      c->multiplyPlainInplace(minusOne);  // a negation either way: no level is spent, no call counted
      EXPECT_TRUE(hip(*c).level() == 3);
      c->multiplyPlainInplace(vec);   // not one number: encoded either way (3 -> 2)
      return c;
    };
    auto on = run(true);
    EXPECT_TRUE(f.constOperandCalls() == 3);
    auto off = run(false);
    EXPECT_TRUE(f.constOperandCalls() == 3);
    EXPECT_TRUE(hip(*on).level() == 2 && hip(*off).level() == 2 && hip(*on).scale() == hip(*off).scale());
    const auto d_on = slotsOf(f, *on), d_off = slotsOf(f, *off);
    for (size_t i = 0; i < x1.size(); ++i) {
      const double want = -(0.3 * (double)x1[i] + 0.1 - 1.0 / 3) * (double)(i + 1);
      if (!(std::fabs(d_on.at(i) - want) <= 1e-3 && std::fabs(d_off.at(i) - want) <= 1e-3 && std::fabs(d_on[i] - d_off[i]) <= 1e-3))
        throw std::runtime_error("slot " + std::to_string(i) + ": on " + std::to_string(d_on[i]) + " off " + std::to_string(d_off[i]) + " want " + std::to_string(want));
    }
    // {50, 30, 50} at scale 2^20: at one limb the product alone, the scale stays squared, and the words are the encoded path's
    HipSchemeConfig small = cfg;
    small.ringDegree = 4096;
    small.ckksBits = {50, 30, 50};
    small.ckksScale = std::ldexp(1.0, 20);
    small.constOperands = true;
    HipCiphertextFactory h(small);
    auto p = h.createCiphertext(x1);
    auto q = p->clone();
    const Cleartext<int> two(std::vector<int>{2});
    p->multiplyPlainInplace(two);
    const double s1 = hip(*p).scale();
    p->multiplyPlainInplace(two);  // nl == 1
    EXPECT_TRUE(h.constOperandCalls() == 2 && hip(*p).level() == 1 && hip(*p).scale() == s1 * h.defaultScale());
    h.setConstOperands(false);
    q->multiplyPlainInplace(two);
    q->multiplyPlainInplace(two);
    EXPECT_TRUE(h.constOperandCalls() == 2 && hip(*p).scale() == hip(*q).scale() && wordsOf(h, *p) == wordsOf(h, *q));
    // a scale that does not fit throws before anything is enqueued: the value keeps its words, level and scale
    HipSchemeConfig wide = small;
    wide.ckksScale = std::ldexp(1.0, 45);  // 2^90 against 80 bits of modulus
    HipCiphertextFactory k(wide);
    auto c = k.createCiphertext(x1);
    const auto before = wordsOf(k, *c);
    EXPECT_THROWS(c->multiplyPlainInplace(two));
    EXPECT_TRUE(k.constOperandCalls() == 0 && hip(*c).level() == 2 && hip(*c).scale() == k.defaultScale() && wordsOf(k, *c) == before);
  });

  t.run("the same as a recorded circuit, replayed on a new input", [&] {
    HipCiphertextFactory f(cfg);
    f.setConstOperands(true);
    CircuitRuntime rt(f, "secret int x = " + listOf(x1) + ";");
    rt.compile(program("a"));
    EXPECT_TRUE(rt.compiled());
    EXPECT_TRUE(f.constOperandCalls() == 8);  // compile interprets twice: eagerly, then into the recording
    for (const auto *xs : {&x1, &x2}) {
      f.setConstOperands(true);
      if (xs == &x2) {
        rt.setInput("x", x2);
        rt.replay();
        EXPECT_TRUE(f.constOperandCalls() == 8);  // a replay dispatches nothing
      }
      f.setConstOperands(false);
      rt.executeAst(program("b"));  // eagerly, from the same input buffer
      auto out = rt.getOutput(kOutputs);
      sameResults(f, out);
      slotsAre(f, named(out, "ya"), *xs);
    }
  });
  t.run("non-dyadic value * scale in a recorded circuit: the same decoded values, replayed on a new input", [&] {
    // the additions sit BEHIND a product, at scale 2^80 / q_3: 2 * scale is no integer, so the encoder may round coefficient 0 one unit
    // away from const_words and the words are not compared -- levels, scales and decoded values are.  z = 4 (3 x + 2 - 5)
    auto prog = [](const std::string &sfx) {
      return "secret int u" + sfx + " = x;\nsecret int z1" + sfx + " = u" + sfx + " *** 3;\nsecret int z2" + sfx + " = z1" + sfx + " +++ 2;\nsecret int z3" + sfx +
             " = z2" + sfx + " --- 5;\nsecret int z" + sfx + " = z3" + sfx + " *** 4;\n";
    };
    HipCiphertextFactory f(cfg);
    f.setConstOperands(true);
    CircuitRuntime rt(f, "secret int x = " + listOf(x1) + ";");
    rt.compile(prog("a"));
    EXPECT_TRUE(rt.compiled() && f.constOperandCalls() == 8);
    for (const auto *xs : {&x1, &x2}) {
      f.setConstOperands(true);
      if (xs == &x2) {
        rt.setInput("x", x2);
        rt.replay();
        EXPECT_TRUE(f.constOperandCalls() == 8);
      }
      f.setConstOperands(false);
      rt.executeAst(prog("b"));
      auto out = rt.getOutput("z2a = z2a; z2b = z2b; za = za; zb = zb;");
      for (const char *v : {"z2", "z"}) {
        auto &a = named(out, std::string(v) + "a"), &b = named(out, std::string(v) + "b");
        EXPECT_TRUE(hip(a).level() == hip(b).level() && hip(a).scale() == hip(b).scale());
      }
      const auto d_on = slotsOf(f, named(out, "za")), d_off = slotsOf(f, named(out, "zb"));
      for (size_t i = 0; i < xs->size(); ++i) {
        const double want = 4.0 * (3.0 * (double)(*xs)[i] - 3.0);
        if (!(std::fabs(d_on.at(i) - want) <= 1e-3 && std::fabs(d_off.at(i) - want) <= 1e-3 && std::fabs(d_on[i] - d_off[i]) <= 1e-3))
          throw std::runtime_error("slot " + std::to_string(i) + ": on " + std::to_string(d_on[i]) + " off " + std::to_string(d_off[i]) + " want " + std::to_string(want));
      }
    }
    // a one-number vector longer than the slots is refused as the encoded path refuses it
    auto c = f.createCiphertext(x1);
    f.setConstOperands(true);
    EXPECT_THROWS(c->addPlainInplace(Cleartext<double>(std::vector<double>(f.usableSlots() + 1, 0.5))));
  });
  return t.summary();
}
