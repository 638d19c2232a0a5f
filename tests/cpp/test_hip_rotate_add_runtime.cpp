// `lhs +++ rotate(v, k)` behind the plugin surface (needs a GPU): the vectorizer's rotate-and-add tree through CircuitRuntime on a
// HipCiphertextFactory with fuseRotateAdd on and off.  The fused path (HipCiphertext::addRotatedInplace -> abc_hip_rotate_add) and
// the separate one (rotateRows + addInplace) must give ciphertexts equal word for word from the same inputs, decrypt to the
// cleartext sum, and the fused run must have issued exactly one fused call per `+++ rotate` pair; the same as a recorded circuit
// and in batch mode.  BFV N = 2^13, CKKS N = 2^14.
#include <string>
#include <vector>

#include "../../include/abc_hip.h"
#include "CircuitRuntime.hpp"
#include "CircuitVectorizer.hpp"
#include "HipCiphertext.hpp"
#include "HipCiphertextFactory.hpp"
#include "mini_test.hpp"

namespace {
std::string listOf(const std::vector<int64_t> &v) {
  std::string s = "{";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "}";
}
size_t count(const std::string &hay, const std::string &needle) {
  size_t n = 0;
  for (size_t at = hay.find(needle); at != std::string::npos; at = hay.find(needle, at + 1)) ++n;
  return n;
}
// the device words of a result
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
int64_t sumOf(const std::vector<int64_t> &v) {
  int64_t s = 0;
  for (auto e : v) s += e;
  return s;
}

// The factory's seeded test encryption draws from one process-wide counter, so two factories never encrypt alike: both paths run on
// ONE factory (setFuseRotateAdd), from the same input ciphertexts -- `secret int xa = x;` is a copy-on-write reference.
struct Tree {
  std::string fused, separate;  // the same program on the copies (xa, suma) and (xb, sumb)
  size_t pairs;
};
Tree makeTree() {
  // sum = sum + x[0] + .. + x[7]: the vectorizer's tree, three `+++ rotate` pairs (4, 2, 1) and a final add
  auto one = [](const std::string &sfx) {
    CircuitVectorizer vz({"sum" + sfx});
    std::string src;
    for (int i = 0; i < 8; ++i) src += "sum" + sfx + " = sum" + sfx + " + x" + sfx + "[" + std::to_string(i) + "];\n";
    std::string prog = vz.vectorize(src);
    for (size_t at = prog.find("__vt0__"); at != std::string::npos; at = prog.find("__vt0__", at)) prog.replace(at, 7, "__vt" + sfx + "__");
    return "secret int x" + sfx + " = x;\nsecret int sum" + sfx + " = sum;\n" + prog;
  };
  Tree t{one("a"), one("b"), 0};
  t.pairs = count(t.fused, "+++ rotate(");
  return t;
}
int64_t slot0(const HipCiphertextFactory &f, AbstractValue &v) {
  std::vector<int64_t> d;
  f.decryptCiphertext(dynamic_cast<AbstractCiphertext &>(v), d);
  return d.at(0);
}

void runScheme(MiniTest &t, const std::string &tag, HipSchemeConfig cfg) {
  const Tree tree = makeTree();
  const std::vector<int64_t> x1 = {3, 1, 4, 1, 5, 9, 2, 6}, x2 = {-7, 10, 0, 25, 8, 8, -3, 1};
  const std::string inputs = "secret int x = " + listOf(x1) + "; secret int sum = {100};";

  t.run((tag + ": the tree, fused against separate").c_str(), [&] {
    EXPECT_TRUE(tree.pairs == 3 && count(tree.separate, "+++ rotate(") == 3);
    HipCiphertextFactory f(cfg);
    EXPECT_TRUE(f.fusesRotateAdd());
    CircuitRuntime rt(f, inputs);
    rt.executeAst(tree.fused);
    EXPECT_TRUE(f.fusedRotateAddCalls() == tree.pairs);
    f.setFuseRotateAdd(false);
    rt.executeAst(tree.separate);
    EXPECT_TRUE(f.fusedRotateAddCalls() == tree.pairs);  // the separate path issues none
    auto out = rt.getOutput("ya = suma; yb = sumb; za = __vta__; zb = __vtb__;");
    EXPECT_TRUE(wordsOf(f, named(out, "ya")) == wordsOf(f, named(out, "yb")));
    EXPECT_TRUE(wordsOf(f, named(out, "za")) == wordsOf(f, named(out, "zb")));
    EXPECT_TRUE(slot0(f, named(out, "ya")) == 100 + sumOf(x1) && slot0(f, named(out, "yb")) == 100 + sumOf(x1));
    // the operation called directly: another operand, a negative step, a NAF step, the same ciphertext as both operands
    auto base = f.createCiphertext(x1), src = f.createCiphertext(x2);
    auto ca = base->clone(), cb = base->clone();
    f.setFuseRotateAdd(true);
    auto &ra = dynamic_cast<RotateAddCapable &>(*ca);
    ra.addRotatedInplace(*src, -2);
    ra.addRotatedInplace(*ca, 1);
    ra.addRotatedInplace(*src, 3);
    EXPECT_TRUE(f.fusedRotateAddCalls() == tree.pairs + 3);
    f.setFuseRotateAdd(false);
    auto &rb = dynamic_cast<RotateAddCapable &>(*cb);
    rb.addRotatedInplace(*src, -2);
    rb.addRotatedInplace(*cb, 1);
    rb.addRotatedInplace(*src, 3);
    EXPECT_TRUE(f.fusedRotateAddCalls() == tree.pairs + 3);
    EXPECT_TRUE(wordsOf(f, *ca) == wordsOf(f, *cb));
    auto want = base->add(*src->rotateRows(-2));  // the plugin's own two calls
    want->addInplace(*want->rotateRows(1));
    want->addInplace(*src->rotateRows(3));
    EXPECT_TRUE(wordsOf(f, *ca) == wordsOf(f, *want));
    // copy-on-write: a clone taken before the operation keeps the old value
    f.setFuseRotateAdd(true);
    auto keep = ca->clone();
    const auto before = wordsOf(f, *keep);
    ra.addRotatedInplace(*src, 1);
    EXPECT_TRUE(wordsOf(f, *keep) == before && wordsOf(f, *ca) != before);
    // the configuration field is what the setter sets
    HipSchemeConfig off = cfg;
    off.fuseRotateAdd = false;
    HipCiphertextFactory g(off);
    EXPECT_TRUE(!g.fusesRotateAdd());
    auto c = g.createCiphertext(x1);
    dynamic_cast<RotateAddCapable &>(*c).addRotatedInplace(*c, 4);
    EXPECT_TRUE(g.fusedRotateAddCalls() == 0 && slot0(g, *c) == x1[0] + x1[4]);
  });

  t.run((tag + ": the same as a recorded circuit, replayed on new inputs").c_str(), [&] {
    HipCiphertextFactory f(cfg);
    CircuitRuntime rt(f, inputs);
    rt.compile(tree.fused);
    EXPECT_TRUE(rt.compiled());
    EXPECT_TRUE(f.fusedRotateAddCalls() == 2 * tree.pairs);  // compile interprets twice: eagerly, then into the recording
    for (const auto *xs : {&x1, &x2}) {
      f.setFuseRotateAdd(true);
      if (xs == &x2) {
        rt.setInput("x", x2);
        rt.replay();
        EXPECT_TRUE(f.fusedRotateAddCalls() == 2 * tree.pairs);  // a replay dispatches nothing
      }
      f.setFuseRotateAdd(false);
      rt.executeAst(tree.separate);  // eagerly, from the same input buffers
      auto out = rt.getOutput("ya = suma; yb = sumb;");
      EXPECT_TRUE(wordsOf(f, named(out, "ya")) == wordsOf(f, named(out, "yb")));
      EXPECT_TRUE(slot0(f, named(out, "ya")) == 100 + sumOf(*xs));
    }
  });

  t.run((tag + ": batch mode, four instances").c_str(), [&] {
    HipSchemeConfig c4 = cfg;
    c4.batch = 4;
    HipCiphertextFactory f(c4);
    const std::vector<std::vector<int64_t>> xs = {x1, x2, {1, 1, 1, 1, 1, 1, 1, 1}, {0, -1, 2, -3, 4, -5, 6, -7}};
    const std::vector<std::vector<int64_t>> sums = {{100}, {0}, {-5}, {7}};
    f.queueBatchedInput(xs);
    f.queueBatchedInput(sums);
    CircuitRuntime rt(f, "secret int x = {0}; secret int sum = {0};");
    rt.executeAst(tree.fused);
    f.setFuseRotateAdd(false);
    rt.executeAst(tree.separate);
    EXPECT_TRUE(f.fusedRotateAddCalls() == tree.pairs);
    auto out = rt.getOutput("ya = suma; yb = sumb;");
    EXPECT_TRUE(wordsOf(f, named(out, "ya")) == wordsOf(f, named(out, "yb")));
    std::vector<std::vector<int64_t>> d;
    f.decryptCiphertextBatch(dynamic_cast<AbstractCiphertext &>(named(out, "ya")), d);
    EXPECT_TRUE(d.size() == 4);
    for (size_t i = 0; i < 4; ++i) EXPECT_TRUE(d[i].at(0) == sums[i][0] + sumOf(xs[i]));
  });
}
}  // namespace

int main() {
  MiniTest t;
  HipSchemeConfig bfv;
  bfv.ringDegree = 8192;
  bfv.seed = 0xABC0ADD1ull;
  runScheme(t, "BFV N=8192", bfv);
  HipSchemeConfig ckks;
  ckks.ckks = true;
  ckks.ringDegree = 16384;
  ckks.seed = 0xABC0ADD2ull;
  runScheme(t, "CKKS N=16384", ckks);
  return t.summary();
}
