// CKKS `x *** p +++ y *** q (+++ ...)` behind the plugin surface (needs a GPU): CircuitRuntime on a HipCiphertextFactory with
// HipSchemeConfig::lazyRescale on and off.  On: exactly one abc_hip_multiply_plain_sum_rescale per recognised run
// (HipCiphertext::plainSum), with the WORDS of that call issued directly on the same operands, one level down, at scale
// sc * ps / q_{nl-1}.  Off (the default): what the plugin issued before the option existed -- one abc_hip_multiply_plain_rescale per
// product and the adds -- word for word, and no new call.  Terms at different levels, a term of all -1 and a value at one limb take
// the calls per term.  40 distinct public values go in two slices (the plaintext cache holds 32), and with the cache full a run of
// its oldest entry and a new value keeps the oldest entry's block alive.  Eagerly, and as a recorded circuit replayed on a new
// input.  On against off the decoded values agree within 1e-3, the tolerance of tests/cpp/test_hip_mulplain_rescale_runtime.cpp.
// N = 4096, {50, 40, 40, 50}, scale 2^40.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/abc_hip.h"
#include "CircuitRuntime.hpp"
#include "HipCiphertext.hpp"
#include "HipCiphertextFactory.hpp"
#include "PlainSumCapable.hpp"
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
AbstractCiphertext &ct(OutputIdentifierValuePairs &out, const std::string &name) { return dynamic_cast<AbstractCiphertext &>(named(out, name)); }
std::vector<double> slots(const HipCiphertextFactory &f, AbstractValue &v, size_t n) {
  std::vector<double> d;
  f.decryptCiphertextReal(dynamic_cast<AbstractCiphertext &>(v), d);
  d.resize(n);
  return d;
}
bool near(const std::vector<double> &got, const std::vector<double> &want, double tol = 1e-3) {
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); ++i)
    if (!(std::fabs(got[i] - want[i]) <= tol)) return false;
  return true;
}

const std::vector<int64_t> x = {1, 2, 3, 4, -5, 6}, y = {10, 20, 30, 40, 50, -60}, u = {2, 2, 3, 3, 0, 1}, p = {2, -3, 4, 0, 7, 1},
                           q = {3, 0, -1, 5, 2, 2}, m = {-1, -1, -1, -1, -1, -1}, x2 = {7, -1, 0, 12, 3, 3};
const std::string INPUTS = "secret int x = " + listOf(x) + "; secret int y = " + listOf(y) + "; secret int u = " + listOf(u) + "; int p = " +
                           listOf(p) + "; int q = " + listOf(q) + "; int m = " + listOf(m) + ";";
const std::string SUM = "x *** p +++ q *** y +++ u *** p";
std::vector<double> weighted(const std::vector<int64_t> &xs) {
  std::vector<double> r(xs.size());
  for (size_t i = 0; i < xs.size(); ++i) r[i] = (double)(xs[i] * p[i] + q[i] * y[i] + u[i] * p[i]);
  return r;
}
std::vector<double> reals(const std::vector<int64_t> &v) { return std::vector<double>(v.begin(), v.end()); }

// ONE abc_hip_multiply_plain_sum_rescale on the operands' own buffers and the factory's plaintexts of `weights` at the operands' level
// and the default scale: the words HipCiphertext::plainSum must give with lazyRescale on (at most 32 terms)
std::vector<uint64_t> direct(const HipCiphertextFactory &f, const std::vector<const AbstractCiphertext *> &cts, const std::vector<std::vector<double>> &weights) {
  const int nl = dynamic_cast<const HipCiphertext &>(*cts[0]).level();
  std::vector<const uint64_t *> a, pl;
  std::vector<std::shared_ptr<const HipCiphertextFactory::DeviceBlock>> held;
  for (size_t k = 0; k < cts.size(); ++k) {
    a.push_back(dynamic_cast<const HipCiphertext &>(*cts[k]).devicePtr());
    held.push_back(f.cachedCkksPlaintextBlock(weights[k], nl, f.defaultScale()));
    pl.push_back(held.back()->p);
  }
  void *d = nullptr;
  const size_t words = f.ciphertextWords(nl - 1);
  abcHipCheck(abc_hip_malloc(f.context(), &d, words * 8), "allocation");
  abcHipCheck(abc_hip_multiply_plain_sum_rescale(f.context(), a.data(), pl.data(), 0, (int)a.size(), nullptr, static_cast<uint64_t *>(d), 2, nl, f.batchSize()),
              "multiply_plain_sum_rescale");
  std::vector<uint64_t> w(words);
  abcHipCheck(abc_hip_memcpy_d2h(f.context(), w.data(), d, words * 8), "download");
  abc_hip_free(f.context(), d);
  return w;
}
}  // namespace

int main() {
  MiniTest t;
  HipSchemeConfig cfg;
  cfg.ckks = true;
  cfg.ringDegree = 4096;
  cfg.ckksBits = {50, 40, 40, 50};
  cfg.seed = 0xABC05CA1ull;
  HipSchemeConfig lazy = cfg;
  lazy.lazyRescale = true;
  const size_t n = x.size();

  t.run("lazyRescale on: one call per run, the words of that call on the same operands", [&] {
    EXPECT_TRUE(!cfg.lazyRescale);  // off by default
    HipCiphertextFactory f(lazy);
    EXPECT_TRUE(f.lazyRescales() && f.fusesPlainSum() && f.plainSumRescaleCalls() == 0);
    CircuitRuntime rt(f, INPUTS);
    rt.executeAst("secret int za = " + SUM + ";");
    EXPECT_TRUE(f.plainSumRescaleCalls() == 1 && f.fusedMultiplyPlainRescaleCalls() == 0 && f.plainSumCalls() == 0);
    auto out = rt.getOutput("za = za; x = x; y = y; u = u;");
    EXPECT_TRUE(dynamic_cast<PlainSumCapable &>(ct(out, "x")).fusePlainSum());
    auto &za = hip(named(out, "za"));
    EXPECT_TRUE(za.level() == 2 && hip(named(out, "x")).level() == 3);
    EXPECT_TRUE(za.scale() == f.defaultScale() * f.defaultScale() / (double)f.prime(2));
    EXPECT_TRUE(near(slots(f, za, n), weighted(x)));
    EXPECT_TRUE(wordsOf(f, za) == direct(f, {&ct(out, "x"), &ct(out, "y"), &ct(out, "u")}, {reals(p), reals(q), reals(p)}));
    // the same run with the option off: other words (a rescale per product), the same values
    f.setLazyRescale(false);
    rt.executeAst("secret int zb = " + SUM + ";");
    EXPECT_TRUE(f.plainSumRescaleCalls() == 1 && f.fusedMultiplyPlainRescaleCalls() == 3);
    auto out2 = rt.getOutput("zb = zb;");
    auto &zb = hip(named(out2, "zb"));
    EXPECT_TRUE(zb.level() == 2 && std::fabs(zb.scale() / za.scale() - 1.0) <= f.scaleTolerance());
    EXPECT_TRUE(near(slots(f, zb, n), weighted(x)) && near(slots(f, zb, n), slots(f, za, n)));
    EXPECT_TRUE(wordsOf(f, zb) != wordsOf(f, za));
    // a sum that goes on: the run is one call, the rest ordinary operations at the new level
    f.setLazyRescale(true);
    rt.executeAst("secret int zc = " + SUM + " +++ za;");
    EXPECT_TRUE(f.plainSumRescaleCalls() == 2);
    auto out3 = rt.getOutput("zc = zc;");
    std::vector<double> twice = weighted(x);
    for (double &v : twice) v *= 2;
    EXPECT_TRUE(near(slots(f, named(out3, "zc"), n), twice));
  });

  t.run("lazyRescale off: the calls the plugin always issued, word for word", [&] {
    HipCiphertextFactory f(cfg);
    EXPECT_TRUE(!f.lazyRescales());
    CircuitRuntime rt(f, INPUTS);
    rt.executeAst("secret int z = " + SUM + ";");
    EXPECT_TRUE(f.plainSumRescaleCalls() == 0 && f.plainSumCalls() == 0 && f.fusedMultiplyPlainRescaleCalls() == 3);
    auto out = rt.getOutput("z = z; x = x; y = y; u = u;");
    EXPECT_TRUE(!dynamic_cast<PlainSumCapable &>(ct(out, "x")).fusePlainSum());
    Cleartext<int> cp(std::vector<int>(p.begin(), p.end())), cq(std::vector<int>(q.begin(), q.end()));
    auto eager = ct(out, "x").multiplyPlain(cp);
    eager->addInplace(*ct(out, "y").multiplyPlain(cq));
    eager->addInplace(*ct(out, "u").multiplyPlain(cp));
    EXPECT_TRUE(wordsOf(f, named(out, "z")) == wordsOf(f, *eager));
    EXPECT_TRUE(hip(named(out, "z")).level() == 2 && hip(named(out, "z")).scale() == hip(*eager).scale());
    EXPECT_TRUE(near(slots(f, named(out, "z"), n), weighted(x)));
    // the operation called directly with the option off: the calls per term
    PlainSumCapable::Terms terms = {{&ct(out, "x"), &cp}, {&ct(out, "y"), &cq}, {&ct(out, "u"), &cp}};
    auto r = dynamic_cast<PlainSumCapable &>(ct(out, "x")).plainSum(terms);
    EXPECT_TRUE(f.plainSumRescaleCalls() == 0 && wordsOf(f, *r) == wordsOf(f, *eager));
    // fusePlainSum off switches the lazy sum off too
    f.setLazyRescale(true);
    f.setFusePlainSum(false);
    EXPECT_TRUE(!dynamic_cast<PlainSumCapable &>(ct(out, "x")).fusePlainSum());
    auto r2 = dynamic_cast<PlainSumCapable &>(ct(out, "x")).plainSum(terms);
    EXPECT_TRUE(f.plainSumRescaleCalls() == 0 && wordsOf(f, *r2) == wordsOf(f, *eager));
  });

  t.run("mixed levels, a term of all -1, one limb and a scale out of bounds: the calls per term", [&] {
    HipCiphertextFactory f(lazy);
    CircuitRuntime rt(f, INPUTS);
    auto perTerm = [&](const PlainSumCapable::Terms &terms) {  // the plugin's own calls, option off
      f.setLazyRescale(false);
      auto r = terms[0].first->multiplyPlain(*terms[0].second);
      for (size_t k = 1; k < terms.size(); ++k) r->addInplace(*terms[k].first->multiplyPlain(*terms[k].second));
      f.setLazyRescale(true);
      return r;
    };
    rt.executeAst("secret int x1 = x *** q;");  // level 2
    auto out = rt.getOutput("x = x; y = y; x1 = x1;");
    EXPECT_TRUE(hip(named(out, "x1")).level() == 2);
    Cleartext<int> cp(std::vector<int>(p.begin(), p.end())), cq(std::vector<int>(q.begin(), q.end())), cm(std::vector<int>(m.begin(), m.end()));
    auto &sum = dynamic_cast<PlainSumCapable &>(ct(out, "x"));
    // a term one level down: multiplyPlain per term, and addInplace brings the products together as it always did
    PlainSumCapable::Terms mixed = {{&ct(out, "x"), &cp}, {&ct(out, "x1"), &cq}};
    size_t fused = f.fusedMultiplyPlainRescaleCalls();
    auto rm = sum.plainSum(mixed);
    EXPECT_TRUE(f.plainSumRescaleCalls() == 0 && f.fusedMultiplyPlainRescaleCalls() == fused + 2);
    EXPECT_TRUE(hip(*rm).level() == 1 && wordsOf(f, *rm) == wordsOf(f, *perTerm(mixed)));
    std::vector<double> wantm(n);
    for (size_t i = 0; i < n; ++i) wantm[i] = (double)(x[i] * p[i] + x[i] * q[i] * q[i]);
    EXPECT_TRUE(near(slots(f, *rm, n), wantm));
    // all -1: multiplyPlain negates there and spends no level
    PlainSumCapable::Terms neg = {{&ct(out, "x"), &cm}, {&ct(out, "y"), &cm}};
    fused = f.fusedMultiplyPlainRescaleCalls();
    auto rn = sum.plainSum(neg);
    EXPECT_TRUE(f.plainSumRescaleCalls() == 0 && f.fusedMultiplyPlainRescaleCalls() == fused);
    EXPECT_TRUE(hip(*rn).level() == 3 && wordsOf(f, *rn) == wordsOf(f, *perTerm(neg)));
    // ... also beside an ordinary term
    PlainSumCapable::Terms half = {{&ct(out, "x"), &cp}, {&ct(out, "y"), &cm}};
    auto rh = sum.plainSum(half);
    EXPECT_TRUE(f.plainSumRescaleCalls() == 0 && hip(*rh).level() == 2 && wordsOf(f, *rh) == wordsOf(f, *perTerm(half)));
    std::vector<double> wantn(n);
    for (size_t i = 0; i < n; ++i) wantn[i] = -(double)(x[i] + y[i]);
    EXPECT_TRUE(near(slots(f, *rn, n), wantn));
    // a scale that does not fit throws before anything is enqueued
    HipSchemeConfig wide = lazy;
    wide.ckksBits = {50, 30, 50};
    wide.ckksScale = std::ldexp(1.0, 45);  // 2^90 against 80 bits of modulus
    HipCiphertextFactory h(wide);
    auto a = h.createCiphertext(x), b = h.createCiphertext(y);
    PlainSumCapable::Terms big = {{a.get(), &cp}, {b.get(), &cq}};
    EXPECT_THROWS(dynamic_cast<PlainSumCapable &>(*a).plainSum(big));
    EXPECT_TRUE(h.plainSumRescaleCalls() == 0 && hip(*a).level() == 2);
    // one limb left: {50, 30, 50} at scale 2^20, after one lazy sum the values sit at one limb
    HipSchemeConfig small = lazy;
    small.ckksBits = {50, 30, 50};
    small.ckksScale = std::ldexp(1.0, 20);
    HipCiphertextFactory g(small);
    auto c = g.createCiphertext(x), d = g.createCiphertext(y);
    PlainSumCapable::Terms two = {{c.get(), &cp}, {d.get(), &cq}};
    auto s1 = dynamic_cast<PlainSumCapable &>(*c).plainSum(two);
    EXPECT_TRUE(g.plainSumRescaleCalls() == 1 && hip(*s1).level() == 1);
    PlainSumCapable::Terms low = {{s1.get(), &cp}, {s1.get(), &cq}};
    auto s2 = dynamic_cast<PlainSumCapable &>(*s1).plainSum(low);
    EXPECT_TRUE(g.plainSumRescaleCalls() == 1 && hip(*s2).level() == 1);  // nl = 1: the products alone, the scale stays squared
    EXPECT_TRUE(hip(*s2).scale() == hip(*s1).scale() * g.defaultScale());
  });

  // 35 distinct public values w0 .. w34
  auto weight = [](int k) { return std::vector<int64_t>{k + 1, 2 - k, 3, k, -1, 2 * k + 1}; };
  std::string publics;
  for (int k = 0; k <= 34; ++k) publics += " int w" + std::to_string(k) + " = " + listOf(weight(k)) + ";";

  t.run("a run longer than the cache goes in slices; the oldest cached plaintext beside a new one", [&] {
    HipCiphertextFactory f(lazy);
    EXPECT_TRUE(HipCiphertextFactory::plainCacheEntries() == 32);
    CircuitRuntime rt(f, INPUTS + publics);
    auto out = rt.getOutput("x = x; y = y;");
    auto &sum = dynamic_cast<PlainSumCapable &>(ct(out, "x"));
    // 40 distinct public values in one run: 32 by abc_hip_multiply_plain_sum at nl, 8 and that sum by the new call
    std::vector<Cleartext<int>> many;
    for (int k = 0; k < 40; ++k) many.emplace_back(std::vector<int>{k + 2, 1, -k, 5, k, 7});
    PlainSumCapable::Terms wide;
    std::vector<double> want(n, 0.0);
    for (int k = 0; k < 40; ++k) {
      wide.emplace_back(&ct(out, k & 1 ? "y" : "x"), &many[k]);
      for (size_t i = 0; i < n; ++i) want[i] += (double)((k & 1 ? y : x)[i] * many[k].getData()[i]);
    }
    auto r = sum.plainSum(wide);
    EXPECT_TRUE(f.plainSumRescaleCalls() == 1 && f.fusedMultiplyPlainRescaleCalls() == 0 && hip(*r).level() == 2);
    EXPECT_TRUE(near(slots(f, *r, n), want));
    f.setLazyRescale(false);
    auto r0 = sum.plainSum(wide);
    f.setLazyRescale(true);
    EXPECT_TRUE(f.fusedMultiplyPlainRescaleCalls() == 40 && near(slots(f, *r0, n), slots(f, *r, n)));
    // fill the cache: w0 .. w31 at this level and scale, w0 its oldest entry
    for (int k = 0; k < 32; ++k) f.cachedCkksPlaintext(reals(weight(k)), 3, f.defaultScale());
    // each round: a hit on the oldest entry, then a miss that evicts it -- the block the hit has just handed out must live on
    for (int round = 0; round < 3; ++round) {
      const int old = round, fresh = 32 + round;
      const std::string z = "s" + std::to_string(round);
      rt.executeAst("secret int " + z + " = x *** w" + std::to_string(old) + " +++ y *** w" + std::to_string(fresh) + ";");
      auto o2 = rt.getOutput(z + " = " + z + ";");
      std::vector<double> pair(n);
      for (size_t i = 0; i < n; ++i) pair[i] = (double)(x[i] * weight(old)[i] + y[i] * weight(fresh)[i]);
      EXPECT_TRUE(near(slots(f, named(o2, z), n), pair));
      EXPECT_TRUE(wordsOf(f, named(o2, z)) == direct(f, {&ct(out, "x"), &ct(out, "y")}, {reals(weight(old)), reals(weight(fresh))}));
    }
    EXPECT_TRUE(f.plainSumRescaleCalls() == 4);
  });

  t.run("the same as a recorded circuit, replayed on a new input", [&] {
    HipCiphertextFactory f(lazy);
    CircuitRuntime rt(f, INPUTS + " secret int z = {0};");
    rt.compile("z = " + SUM + ";");
    EXPECT_TRUE(rt.compiled());
    EXPECT_TRUE(f.plainSumRescaleCalls() == 2);  // compile interprets twice: eagerly, then into the recording
    auto out = rt.getOutput("z = z; x = x; y = y; u = u;");
    EXPECT_TRUE(near(slots(f, named(out, "z"), n), weighted(x)));
    EXPECT_TRUE(wordsOf(f, named(out, "z")) == direct(f, {&ct(out, "x"), &ct(out, "y"), &ct(out, "u")}, {reals(p), reals(q), reals(p)}));
    rt.setInput("x", x2);
    rt.replay();
    EXPECT_TRUE(f.plainSumRescaleCalls() == 2);  // a replay dispatches nothing
    out = rt.getOutput("z = z; x = x; y = y; u = u;");
    EXPECT_TRUE(near(slots(f, named(out, "x"), n), reals(x2)));
    EXPECT_TRUE(near(slots(f, named(out, "z"), n), weighted(x2)));
    EXPECT_TRUE(hip(named(out, "z")).level() == 2);
    EXPECT_TRUE(wordsOf(f, named(out, "z")) == direct(f, {&ct(out, "x"), &ct(out, "y"), &ct(out, "u")}, {reals(p), reals(q), reals(p)}));
  });
  return t.summary();
}
