// `x *** y +++ u *** v (+++ ...)` behind the plugin surface (needs a GPU): CircuitRuntime on a HipCiphertextFactory with
// HipSchemeConfig::lazyRelinearize on and off.  On: exactly one abc_hip_mul_sum_relin per recognised run (HipCiphertext::mulSum),
// and the result decodes to the values the per-product sequence decodes to -- its words differ, which is why the option is off by
// default.  Off: the words are those of the plugin's own multiply and addInplace, as before.  The same program as a recorded circuit,
// replayed on new inputs.  BFVDefault(4096) and the CKKS factory.
#include <string>
#include <vector>

#include "../../include/abc_hip.h"
#include "CircuitRuntime.hpp"
#include "HipCiphertext.hpp"
#include "HipCiphertextFactory.hpp"
#include "MulSumCapable.hpp"
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
std::vector<int64_t> sumOfProducts(const std::vector<int64_t> &x, const std::vector<int64_t> &y, const std::vector<int64_t> &u,
                                   const std::vector<int64_t> &v, const std::vector<int64_t> &w) {
  std::vector<int64_t> r(x.size());
  for (size_t i = 0; i < x.size(); ++i) r[i] = x[i] * y[i] + u[i] * v[i] + w[i] * x[i];
  return r;
}

void runScheme(MiniTest &t, const std::string &tag, HipSchemeConfig cfg) {
  const std::vector<int64_t> x = {1, 2, 3, 4, -5, 6}, y = {10, 20, 30, 40, 50, -60}, u = {2, 2, 3, 3, 0, 1}, v = {5, 6, 7, 8, 9, 10},
                             w = {1, 0, 1, 0, -2, 3}, x2 = {7, -1, 0, 12, 3, 3};
  const std::string inputs = "secret int x = " + listOf(x) + "; secret int y = " + listOf(y) + "; secret int u = " + listOf(u) +
                             "; secret int v = " + listOf(v) + "; secret int w = " + listOf(w) + ";";
  const std::string sum = "x *** y +++ u *** v +++ w *** x";
  const size_t n = x.size();

  t.run((tag + ": on against off").c_str(), [&] {
    HipSchemeConfig on = cfg;
    on.lazyRelinearize = true;
    HipCiphertextFactory f(on);
    EXPECT_TRUE(f.lazyRelinearizes());
    CircuitRuntime rt(f, inputs);
    rt.executeAst("secret int za = " + sum + ";");
    EXPECT_TRUE(f.mulSumCalls() == 1);  // one call for the run of three
    rt.executeAst("secret int zc = " + sum + " +++ w;");
    EXPECT_TRUE(f.mulSumCalls() == 2);  // the run, then an ordinary add
    f.setLazyRelinearize(false);
    rt.executeAst("secret int zb = " + sum + ";");
    EXPECT_TRUE(f.mulSumCalls() == 2);  // off: none
    auto out = rt.getOutput("za = za; zb = zb; zc = zc; x = x; y = y; u = u; v = v; w = w;");
    const auto want = sumOfProducts(x, y, u, v, w);
    EXPECT_TRUE(head(f, named(out, "za"), n) == want);
    EXPECT_TRUE(head(f, named(out, "zb"), n) == want);
    auto wantc = want;
    for (size_t i = 0; i < n; ++i) wantc[i] += w[i];
    EXPECT_TRUE(head(f, named(out, "zc"), n) == wantc);
    // off: the words of the plugin's own calls, as before the option existed
    auto eager = ct(out, "x").multiply(ct(out, "y"));
    eager->addInplace(*ct(out, "u").multiply(ct(out, "v")));
    eager->addInplace(*ct(out, "w").multiply(ct(out, "x")));
    EXPECT_TRUE(wordsOf(f, named(out, "zb")) == wordsOf(f, *eager));
    // on: another ciphertext (one key switch, not three) at the same level
    EXPECT_TRUE(dynamic_cast<HipCiphertext &>(named(out, "za")).level() == dynamic_cast<HipCiphertext &>(named(out, "zb")).level());
    EXPECT_TRUE(wordsOf(f, named(out, "za")) != wordsOf(f, named(out, "zb")));
    // the operation called directly, a square among the terms; with the option off it takes the calls per term
    f.setLazyRelinearize(true);
    auto &lazy = dynamic_cast<MulSumCapable &>(ct(out, "x"));
    const MulSumCapable::Terms terms = {{&ct(out, "x"), &ct(out, "x")}, {&ct(out, "u"), &ct(out, "v")}};
    auto r1 = lazy.mulSum(terms);
    EXPECT_TRUE(f.mulSumCalls() == 3);
    f.setLazyRelinearize(false);
    auto r2 = lazy.mulSum(terms);
    EXPECT_TRUE(f.mulSumCalls() == 3);
    std::vector<int64_t> sq(n);
    for (size_t i = 0; i < n; ++i) sq[i] = x[i] * x[i] + u[i] * v[i];
    EXPECT_TRUE(head(f, *r1, n) == sq && head(f, *r2, n) == sq);
    // the default is off
    HipCiphertextFactory g(cfg);
    EXPECT_TRUE(!g.lazyRelinearizes());
    CircuitRuntime rg(g, inputs);
    rg.executeAst("secret int z = " + sum + ";");
    EXPECT_TRUE(g.mulSumCalls() == 0);
    auto og = rg.getOutput("z = z;");
    EXPECT_TRUE(head(g, named(og, "z"), n) == want);
  });

  t.run((tag + ": the same as a recorded circuit, replayed on new inputs").c_str(), [&] {
    HipSchemeConfig on = cfg;
    on.lazyRelinearize = true;
    HipCiphertextFactory f(on);
    CircuitRuntime rt(f, inputs + " secret int z = {0};");
    rt.compile("z = " + sum + ";");
    EXPECT_TRUE(rt.compiled());
    EXPECT_TRUE(f.mulSumCalls() == 2);  // compile interprets twice: eagerly, then into the recording
    auto out = rt.getOutput("z = z;");
    EXPECT_TRUE(head(f, named(out, "z"), n) == sumOfProducts(x, y, u, v, w));
    rt.setInput("x", x2);
    rt.replay();
    EXPECT_TRUE(f.mulSumCalls() == 2);  // a replay dispatches nothing
    out = rt.getOutput("z = z;");
    EXPECT_TRUE(head(f, named(out, "z"), n) == sumOfProducts(x2, y, u, v, w));
  });
}
}  // namespace

int main() {
  MiniTest t;
  HipSchemeConfig bfv;
  bfv.ringDegree = 4096;
  bfv.seed = 0xABC0511Aull;
  runScheme(t, "BFV N=4096", bfv);
  HipSchemeConfig ckks;
  ckks.ckks = true;
  ckks.ringDegree = 16384;
  ckks.seed = 0xABC0511Bull;
  runScheme(t, "CKKS N=16384", ckks);
  return t.summary();
}
