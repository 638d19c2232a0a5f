// `x *** p +++ y *** q (+++ ...)` behind the plugin surface (needs a GPU): CircuitRuntime on a HipCiphertextFactory with
// HipSchemeConfig::fusePlainSum on and off.  On (the default, BFV): exactly one abc_hip_bfv_multiply_plain_sum per recognised run
// (HipCiphertext::plainSum), and the result has the WORDS of the plugin's own multiplyPlain and addInplace -- which is why the option
// is on by default.  A term whose public value is all -1 sends the whole run to the calls per term; 40 terms go in two calls (the
// plaintext cache holds 32).  With the cache full, a run of its oldest entry and a new value: the entry's block must outlive the eviction
// the new value causes.  The same programs as recorded circuits, replayed on new inputs.  BFVDefault(4096); the CKKS factory
// offers the interface and never fuses.
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
std::vector<uint64_t> wordsOf(const HipCiphertextFactory &f, AbstractValue &v) {
  auto &c = dynamic_cast<HipCiphertext &>(v);
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
std::vector<int64_t> head(const HipCiphertextFactory &f, AbstractValue &v, size_t n) {
  std::vector<int64_t> d;
  f.decryptCiphertext(dynamic_cast<AbstractCiphertext &>(v), d);
  d.resize(n);
  return d;
}

const std::vector<int64_t> x = {1, 2, 3, 4, -5, 6}, y = {10, 20, 30, 40, 50, -60}, u = {2, 2, 3, 3, 0, 1}, p = {2, -3, 4, 0, 7, 1},
                           q = {3, 0, -1, 5, 2, 2}, m = {-1, -1, -1, -1, -1, -1}, x2 = {7, -1, 0, 12, 3, 3};
const std::string INPUTS = "secret int x = " + listOf(x) + "; secret int y = " + listOf(y) + "; secret int u = " + listOf(u) + "; int p = " +
                           listOf(p) + "; int q = " + listOf(q) + "; int m = " + listOf(m) + ";";
const std::string SUM = "x *** p +++ q *** y +++ u *** p";
std::vector<int64_t> weighted(const std::vector<int64_t> &xs) {
  std::vector<int64_t> r(xs.size());
  for (size_t i = 0; i < xs.size(); ++i) r[i] = xs[i] * p[i] + q[i] * y[i] + u[i] * p[i];
  return r;
}
}  // namespace

int main() {
  MiniTest t;
  HipSchemeConfig bfv;
  bfv.ringDegree = 4096;
  bfv.seed = 0xABC0511Cull;
  const size_t n = x.size();

  t.run("BFV N=4096: on against off, word for word", [&] {
    HipCiphertextFactory f(bfv);
    EXPECT_TRUE(f.fusesPlainSum());  // the default
    CircuitRuntime rt(f, INPUTS);
    rt.executeAst("secret int za = " + SUM + ";");
    EXPECT_TRUE(f.plainSumCalls() == 1);  // one call for the run of three
    rt.executeAst("secret int zc = " + SUM + " +++ u;");
    EXPECT_TRUE(f.plainSumCalls() == 2);  // the run, then an ordinary add
    rt.executeAst("secret int zm = x *** m +++ q *** y;");
    EXPECT_TRUE(f.plainSumCalls() == 2);  // a term of all -1: the calls per term (multiplyPlain negates there)
    f.setFusePlainSum(false);
    rt.executeAst("secret int zb = " + SUM + "; secret int zd = " + SUM + " +++ u; secret int zn = x *** m +++ q *** y;");
    EXPECT_TRUE(f.plainSumCalls() == 2);  // off: none
    auto out = rt.getOutput("za = za; zb = zb; zc = zc; zd = zd; zm = zm; zn = zn; x = x; y = y; u = u;");
    const auto want = weighted(x);
    EXPECT_TRUE(head(f, named(out, "za"), n) == want);
    EXPECT_TRUE(head(f, named(out, "zb"), n) == want);
    EXPECT_TRUE(wordsOf(f, named(out, "za")) == wordsOf(f, named(out, "zb")));
    EXPECT_TRUE(wordsOf(f, named(out, "zc")) == wordsOf(f, named(out, "zd")));
    EXPECT_TRUE(wordsOf(f, named(out, "zm")) == wordsOf(f, named(out, "zn")));
    std::vector<int64_t> wantm(n);
    for (size_t i = 0; i < n; ++i) wantm[i] = -x[i] + q[i] * y[i];
    EXPECT_TRUE(head(f, named(out, "zm"), n) == wantm);
    // off is the plugin's own calls, as before the option existed
    Cleartext<int> cp(std::vector<int>(p.begin(), p.end())), cq(std::vector<int>(q.begin(), q.end()));
    auto eager = ct(out, "x").multiplyPlain(cp);
    eager->addInplace(*ct(out, "y").multiplyPlain(cq));
    eager->addInplace(*ct(out, "u").multiplyPlain(cp));
    EXPECT_TRUE(wordsOf(f, named(out, "zb")) == wordsOf(f, *eager));
    // the operation called directly: forty terms of ten distinct public values go in two calls, the second with the first's sum as addend
    f.setFusePlainSum(true);
    auto &sum = dynamic_cast<PlainSumCapable &>(ct(out, "x"));
    EXPECT_TRUE(sum.fusePlainSum());
    std::vector<Cleartext<int>> weights;
    for (int k = 0; k < 10; ++k) weights.emplace_back(std::vector<int>{k + 1, -k, 3, k * k, 1, 2});
    PlainSumCapable::Terms terms;
    for (int k = 0; k < 40; ++k) terms.emplace_back(&ct(out, k % 3 == 0 ? "x" : k % 3 == 1 ? "y" : "u"), &weights[k % 10]);
    const size_t before = f.plainSumCalls();
    auto r1 = sum.plainSum(terms);
    EXPECT_TRUE(f.plainSumCalls() == before + 2);
    f.setFusePlainSum(false);
    auto r2 = sum.plainSum(terms);
    EXPECT_TRUE(f.plainSumCalls() == before + 2);
    EXPECT_TRUE(wordsOf(f, *r1) == wordsOf(f, *r2));
    // more distinct public values than the cache holds, in one run: slices of 32
    f.setFusePlainSum(true);
    std::vector<Cleartext<int>> many;
    for (int k = 0; k < 40; ++k) many.emplace_back(std::vector<int>{k + 2, 1, -k, 5, k, 7});
    PlainSumCapable::Terms wide;
    for (int k = 0; k < 40; ++k) wide.emplace_back(&ct(out, k & 1 ? "y" : "x"), &many[k]);
    auto r3 = sum.plainSum(wide);
    f.setFusePlainSum(false);
    auto r4 = sum.plainSum(wide);
    EXPECT_TRUE(wordsOf(f, *r3) == wordsOf(f, *r4));
  });

  t.run("BFV N=4096: the same as a recorded circuit, replayed on new inputs", [&] {
    // recorded with the option on and with it off: after a replay on new inputs either result has the words of the plugin's own
    // multiplyPlain and addInplace on those inputs (each factory encrypts for itself, so the two are compared through that sequence)
    for (int on = 1; on >= 0; --on) {
      HipSchemeConfig cfg = bfv;
      cfg.fusePlainSum = on != 0;
      HipCiphertextFactory f(cfg);
      CircuitRuntime rt(f, INPUTS + " secret int z = {0};");
      rt.compile("z = " + SUM + ";");
      EXPECT_TRUE(rt.compiled());
      EXPECT_TRUE(f.plainSumCalls() == (on ? 2u : 0u));  // compile interprets twice: eagerly, then into the recording
      auto out = rt.getOutput("z = z;");
      EXPECT_TRUE(head(f, named(out, "z"), n) == weighted(x));
      rt.setInput("x", x2);
      rt.replay();
      EXPECT_TRUE(f.plainSumCalls() == (on ? 2u : 0u));  // a replay dispatches nothing
      out = rt.getOutput("z = z; x = x; y = y; u = u;");
      EXPECT_TRUE(head(f, named(out, "z"), n) == weighted(x2));
      EXPECT_TRUE(head(f, named(out, "x"), n) == x2);
      f.setFusePlainSum(false);
      Cleartext<int> cp(std::vector<int>(p.begin(), p.end())), cq(std::vector<int>(q.begin(), q.end()));
      auto eager = ct(out, "x").multiplyPlain(cp);
      eager->addInplace(*ct(out, "y").multiplyPlain(cq));
      eager->addInplace(*ct(out, "u").multiplyPlain(cp));
      EXPECT_TRUE(wordsOf(f, named(out, "z")) == wordsOf(f, *eager));
    }
  });

  // 33 distinct public values w0 .. w32, the first 32 used pairwise so that the cache of NTT-form plaintexts is full with w0 its oldest entry
  auto weight = [](int k) { return std::vector<int64_t>{k + 1, 2 - k, 3, k, -1, 2 * k + 1}; };
  std::string publics, fill;
  for (int k = 0; k <= 34; ++k) publics += " int w" + std::to_string(k) + " = " + listOf(weight(k)) + ";";
  for (int k = 0; k < 32; k += 2)
    fill += "secret int t" + std::to_string(k) + " = x *** w" + std::to_string(k) + " +++ y *** w" + std::to_string(k + 1) + ";";
  auto pair = [&](const std::vector<int64_t> &xs, int a, int b) {
    std::vector<int64_t> r(n);
    for (size_t i = 0; i < n; ++i) r[i] = xs[i] * weight(a)[i] + y[i] * weight(b)[i];
    return r;
  };
  auto perTerm = [&](HipCiphertextFactory &f, OutputIdentifierValuePairs &out, int a, int b) {  // the plugin's own calls, option off
    const bool was = f.fusesPlainSum();
    f.setFusePlainSum(false);
    const auto wa = weight(a), wb = weight(b);
    Cleartext<int> ca(std::vector<int>(wa.begin(), wa.end())), cb(std::vector<int>(wb.begin(), wb.end()));
    auto r = ct(out, "x").multiplyPlain(ca);
    r->addInplace(*ct(out, "y").multiplyPlain(cb));
    f.setFusePlainSum(was);
    return r;
  };

  t.run("BFV N=4096: the oldest cached plaintext beside a new one, with the cache full", [&] {
    HipCiphertextFactory f(bfv);
    EXPECT_TRUE(HipCiphertextFactory::plainCacheEntries() == 32);
    CircuitRuntime rt(f, INPUTS + publics);
    rt.executeAst(fill);
    EXPECT_TRUE(f.plainSumCalls() == 16);
    // each round: a hit on the least recently used entry, then a miss that evicts -- never the block the hit has just handed out
    const int oldest[3] = {0, 2, 4};  // after round r the miss has evicted w(2r + 1)
    for (int r = 0; r < 3; ++r) {
      const std::string z = "s" + std::to_string(r);
      rt.executeAst("secret int " + z + " = x *** w" + std::to_string(oldest[r]) + " +++ y *** w" + std::to_string(32 + r) + ";");
      auto out = rt.getOutput(z + " = " + z + "; x = x; y = y;");
      EXPECT_TRUE(head(f, named(out, z), n) == pair(x, oldest[r], 32 + r));
      EXPECT_TRUE(wordsOf(f, named(out, z)) == wordsOf(f, *perTerm(f, out, oldest[r], 32 + r)));
    }
    EXPECT_TRUE(f.plainSumCalls() == 19);
  });

  t.run("BFV N=4096: the same inside a recorded circuit", [&] {
    HipCiphertextFactory f(bfv);
    CircuitRuntime rt(f, INPUTS + publics + " secret int z = {0};");
    rt.executeAst(fill);
    rt.compile("z = x *** w0 +++ y *** w32;");  // eagerly: a hit on the oldest entry and a miss; recorded: two hits
    EXPECT_TRUE(rt.compiled());
    auto out = rt.getOutput("z = z; x = x; y = y;");
    EXPECT_TRUE(head(f, named(out, "z"), n) == pair(x, 0, 32));
    EXPECT_TRUE(wordsOf(f, named(out, "z")) == wordsOf(f, *perTerm(f, out, 0, 32)));
    rt.setInput("x", x2);
    rt.replay();
    out = rt.getOutput("z = z; x = x; y = y;");
    EXPECT_TRUE(head(f, named(out, "z"), n) == pair(x2, 0, 32));
    EXPECT_TRUE(wordsOf(f, named(out, "z")) == wordsOf(f, *perTerm(f, out, 0, 32)));
  });

  t.run("CKKS: the interface is offered and never fuses", [&] {
    HipSchemeConfig ckks;
    ckks.ckks = true;
    ckks.ringDegree = 16384;
    ckks.seed = 0xABC0511Dull;
    HipCiphertextFactory f(ckks);
    CircuitRuntime rt(f, INPUTS);
    rt.executeAst("secret int z = " + SUM + ";");
    EXPECT_TRUE(f.plainSumCalls() == 0);
    auto out = rt.getOutput("z = z; x = x;");
    EXPECT_TRUE(!dynamic_cast<PlainSumCapable &>(ct(out, "x")).fusePlainSum());
    EXPECT_TRUE(head(f, named(out, "z"), n) == weighted(x));
  });
  return t.summary();
}
