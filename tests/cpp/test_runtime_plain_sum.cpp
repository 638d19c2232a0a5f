// CircuitRuntime::additive's peephole for sums of ciphertext-by-public-value products, on a recording fake backend: a run
// `x *** p +++ y *** q (+++ ...)` of two or more products, each of one declared secret and one declared non-secret variable in either
// order, becomes ONE PlainSumCapable::plainSum -- terms in the order written, the ciphertext first in each -- when the first
// ciphertext offers the interface and fusePlainSum() says so; every other shape, a backend without the interface and one with the
// option off issue what they always issued.  The decoded values are the same either way, on the fakes and on the Dummy backend.
#include <string>
#include <vector>

#include "CircuitRuntime.hpp"
#include "DummyCiphertextFactory.hpp"
#include "MulSumCapable.hpp"
#include "PlainSumCapable.hpp"
#include "mini_test.hpp"

namespace {
std::vector<std::string> opLog;  // what the backend was asked to do, in order
enum Mode { Plain, FuseOff, FuseOn };

class FakeBase : public AbstractCiphertext {
 protected:
  [[noreturn]] static void no(const char *what) { throw std::runtime_error(std::string("fake backend: ") + what); }
  virtual std::unique_ptr<FakeBase> copy() const = 0;

 public:
  static const std::vector<int64_t> &dataOf(const AbstractCiphertext &c) { return dynamic_cast<const FakeBase &>(c).values; }
  std::vector<int64_t> values;
  explicit FakeBase(const std::reference_wrapper<const AbstractCiphertextFactory> f) : AbstractCiphertext(f) {}
  std::unique_ptr<AbstractCiphertext> multiply(const AbstractCiphertext &o) const override { auto r = copy(); r->multiplyInplace(o); return r; }
  void multiplyInplace(const AbstractCiphertext &o) override {
    opLog.push_back("mul");
    for (size_t i = 0; i < values.size(); ++i) values[i] *= dataOf(o)[i];
  }
  std::unique_ptr<AbstractCiphertext> multiplyPlain(const ICleartext &o) const override { auto r = copy(); r->multiplyPlainInplace(o); return r; }
  void multiplyPlainInplace(const ICleartext &o) override {
    opLog.push_back("mul_plain");
    const auto &p = dynamic_cast<const Cleartext<int> &>(o).getData();
    for (size_t i = 0; i < values.size(); ++i) values[i] *= p[p.size() == 1 ? 0 : i];
  }
  std::unique_ptr<AbstractCiphertext> add(const AbstractCiphertext &o) const override { auto r = copy(); r->addInplace(o); return r; }
  void addInplace(const AbstractCiphertext &o) override {
    opLog.push_back("add");
    for (size_t i = 0; i < values.size(); ++i) values[i] += dataOf(o)[i];
  }
  std::unique_ptr<AbstractCiphertext> addPlain(const ICleartext &) const override { no("addPlain"); }
  void addPlainInplace(const ICleartext &) override { no("addPlainInplace"); }
  std::unique_ptr<AbstractCiphertext> subtract(const AbstractCiphertext &o) const override { auto r = copy(); r->subtractInplace(o); return r; }
  void subtractInplace(const AbstractCiphertext &o) override {
    opLog.push_back("sub");
    for (size_t i = 0; i < values.size(); ++i) values[i] -= dataOf(o)[i];
  }
  std::unique_ptr<AbstractCiphertext> subtractPlain(const ICleartext &) const override { no("subtractPlain"); }
  void subtractPlainInplace(const ICleartext &) override { no("subtractPlainInplace"); }
  std::unique_ptr<AbstractCiphertext> rotateRows(int) const override { no("rotateRows"); }
  void rotateRowsInplace(int) override { no("rotateRowsInplace"); }
  std::unique_ptr<AbstractCiphertext> clone() const override { return copy(); }

  void add_inplace(const AbstractValue &o) override { addInplace(dynamic_cast<const AbstractCiphertext &>(o)); }
  void subtract_inplace(const AbstractValue &o) override { subtractInplace(dynamic_cast<const AbstractCiphertext &>(o)); }
  void multiply_inplace(const AbstractValue &o) override {
    if (auto c = dynamic_cast<const AbstractCiphertext *>(&o)) multiplyInplace(*c);
    else multiplyPlainInplace(dynamic_cast<const ICleartext &>(o));
  }
  void divide_inplace(const AbstractValue &) override { no("divide"); }
  void modulo_inplace(const AbstractValue &) override { no("modulo"); }
  void logicalAnd_inplace(const AbstractValue &) override { no("logicalAnd"); }
  void logicalOr_inplace(const AbstractValue &) override { no("logicalOr"); }
  void logicalLess_inplace(const AbstractValue &) override { no("logicalLess"); }
  void logicalLessEqual_inplace(const AbstractValue &) override { no("logicalLessEqual"); }
  void logicalGreater_inplace(const AbstractValue &) override { no("logicalGreater"); }
  void logicalGreaterEqual_inplace(const AbstractValue &) override { no("logicalGreaterEqual"); }
  void logicalEqual_inplace(const AbstractValue &) override { no("logicalEqual"); }
  void logicalNotEqual_inplace(const AbstractValue &) override { no("logicalNotEqual"); }
  void logicalNot_inplace() override { no("logicalNot"); }
  void bitwiseAnd_inplace(const AbstractValue &) override { no("bitwiseAnd"); }
  void bitwiseXor_inplace(const AbstractValue &) override { no("bitwiseXor"); }
  void bitwiseOr_inplace(const AbstractValue &) override { no("bitwiseOr"); }
  void bitwiseNot_inplace() override { no("bitwiseNot"); }
};

class PlainFake : public FakeBase {
  std::unique_ptr<FakeBase> copy() const override { return std::make_unique<PlainFake>(*this); }

 public:
  using FakeBase::FakeBase;
};
template <bool On>
class SumFake : public FakeBase, public PlainSumCapable {
  std::unique_ptr<FakeBase> copy() const override { return std::make_unique<SumFake>(*this); }

 public:
  using FakeBase::FakeBase;
  bool fusePlainSum() const override { return On; }
  std::unique_ptr<AbstractCiphertext> plainSum(const Terms &terms) const override {
    if (terms.empty() || terms[0].first != this) no("plainSum: the first ciphertext is the receiver");
    std::string entry = "plain_sum " + std::to_string(terms.size()) + ":";  // with each term's operands: ciphertext head * plaintext head
    auto r = std::make_unique<SumFake>(*this);
    for (auto &v : r->values) v = 0;
    for (const auto &t : terms) {
      const auto &p = dynamic_cast<const Cleartext<int> &>(*t.second).getData();
      entry += " " + std::to_string(dataOf(*t.first)[0]) + "*" + std::to_string(p[0]);
      for (size_t i = 0; i < r->values.size(); ++i) r->values[i] += dataOf(*t.first)[i] * p[p.size() == 1 ? 0 : i];
    }
    opLog.push_back(entry);
    return r;
  }
};

template <class Ct>
class FakeFactory : public AbstractCiphertextFactory {
 public:
  std::unique_ptr<AbstractCiphertext> createCiphertext(const std::vector<int64_t> &data) const override {
    auto c = std::make_unique<Ct>(std::cref<AbstractCiphertextFactory>(*this));
    c->values = data;
    return c;
  }
  std::unique_ptr<AbstractCiphertext> createCiphertext(const std::vector<int> &data) const override {
    return createCiphertext(std::vector<int64_t>(data.begin(), data.end()));
  }
  std::unique_ptr<AbstractCiphertext> createCiphertext(int64_t data) const override { return createCiphertext(std::vector<int64_t>{data}); }
  std::unique_ptr<AbstractCiphertext> createCiphertext(std::unique_ptr<AbstractValue> &&v) const override {
    if (auto c = dynamic_cast<Cleartext<int> *>(v.get())) return createCiphertext(c->getData());
    throw std::runtime_error("fake backend: createCiphertext of this value");
  }
  void decryptCiphertext(AbstractCiphertext &c, std::vector<int64_t> &out) const override { out = dynamic_cast<FakeBase &>(c).values; }
  std::string getString(AbstractCiphertext &) const override { return "fake"; }
};

const char *INPUTS = "secret int x = {1, 2, 3, 4}; secret int y = {10, 20, 30, 40}; secret int u = {2, 2, 3, 3}; "
                     "secret int z = {0, 0, 0, 0}; int p = {2, 2, 2, 2}; int q = {3, 0, 1, 5}; int m = {-1, -1, -1, -1};";

struct Outcome {
  std::vector<std::string> ops;
  std::vector<int64_t> z;
};
template <class Factory>
Outcome runOn(Factory &f, const std::string &program) {
  CircuitRuntime rt(f, INPUTS);
  opLog.clear();
  rt.executeAst(program);
  Outcome o;
  auto out = rt.getOutput("r = z;");
  f.decryptCiphertext(dynamic_cast<AbstractCiphertext &>(*out.at(0).second), o.z);
  o.ops = opLog;
  return o;
}
Outcome run(Mode m, const std::string &program) {
  if (m == FuseOn) { FakeFactory<SumFake<true>> f; return runOn(f, program); }
  if (m == FuseOff) { FakeFactory<SumFake<false>> f; return runOn(f, program); }
  FakeFactory<PlainFake> f;
  return runOn(f, program);
}
using Ops = std::vector<std::string>;

// with the interface offered and on the program issues `fused`; offered but off, and not offered, `eager`; the same z everywhere
void expectOps(const std::string &program, const Ops &fused, const Ops &eager, const std::vector<int64_t> &z) {
  auto join = [](const Ops &v) { std::string s; for (auto &e : v) s += "[" + e + "]"; return s; };
  for (Mode m : {FuseOn, FuseOff, Plain}) {
    const Outcome o = run(m, program);
    const Ops &want = m == FuseOn ? fused : eager;
    if (o.ops != want) throw std::runtime_error(program + " in mode " + std::to_string(m) + " issued " + join(o.ops) + ", want " + join(want));
    if (o.z != z) throw std::runtime_error(program + " in mode " + std::to_string(m) + " gave " + vecToString(o.z) + ", want " + vecToString(z));
  }
}
}  // namespace

int main() {
  MiniTest t;
  const Ops two = {"mul_plain", "mul_plain", "add"}, three = {"mul_plain", "mul_plain", "add", "mul_plain", "add"};
  t.run("a run of products with public values is one plain_sum when offered and asked for; operands in the order written", [&] {
    expectOps("z = x *** p +++ y *** q;", {"plain_sum 2: 1*2 10*3"}, two, {32, 4, 36, 208});
    expectOps("z = x * p + y * q;", {"plain_sum 2: 1*2 10*3"}, two, {32, 4, 36, 208});
    expectOps("z = p *** x +++ y *** q;", {"plain_sum 2: 1*2 10*3"}, two, {32, 4, 36, 208});  // the public factor first
    expectOps("z = p *** x +++ q *** y;", {"plain_sum 2: 1*2 10*3"}, two, {32, 4, 36, 208});
    expectOps("z = y *** q +++ x *** p;", {"plain_sum 2: 10*3 1*2"}, two, {32, 4, 36, 208});
    expectOps("z = x *** p +++ y *** q +++ u *** p;", {"plain_sum 3: 1*2 10*3 2*2"}, three, {36, 8, 42, 214});
    expectOps("z = x *** p +++ x *** q;", {"plain_sum 2: 1*2 1*3"}, two, {5, 4, 9, 28});  // one ciphertext twice
    expectOps("z = x *** p +++ y *** p;", {"plain_sum 2: 1*2 10*2"}, two, {22, 44, 66, 88});  // one public value twice
    expectOps("z = x *** m +++ y *** q;", {"plain_sum 2: 1*-1 10*3"}, two, {29, -2, 27, 196});  // all -1: the BACKEND's to fall back on
    expectOps("secret int s = x *** p +++ y *** q; z = s;", {"plain_sum 2: 1*2 10*3"}, two, {32, 4, 36, 208});
    // what follows the run is added, subtracted or multiplied as it always was
    expectOps("z = x *** p +++ y *** q +++ u;", {"plain_sum 2: 1*2 10*3", "add"}, {"mul_plain", "mul_plain", "add", "add"}, {34, 6, 39, 211});
    expectOps("z = x *** p +++ y *** q --- u *** p;", {"plain_sum 2: 1*2 10*3", "mul_plain", "sub"},
              {"mul_plain", "mul_plain", "add", "mul_plain", "sub"}, {28, 0, 30, 202});
    expectOps("z = (x *** p +++ y *** q) *** u;", {"plain_sum 2: 1*2 10*3", "mul"}, {"mul_plain", "mul_plain", "add", "mul"}, {64, 8, 108, 624});
    // a product that does not qualify ends the run in front of it
    expectOps("z = x *** p +++ y *** q +++ u *** p *** q;", {"plain_sum 2: 1*2 10*3", "mul_plain", "mul_plain", "add"},
              {"mul_plain", "mul_plain", "add", "mul_plain", "mul_plain", "add"}, {44, 4, 42, 238});
    expectOps("z = x *** p +++ y *** q +++ u *** y;", {"plain_sum 2: 1*2 10*3", "mul", "add"}, {"mul_plain", "mul_plain", "add", "mul", "add"},
              {52, 44, 126, 328});
  });
  t.run("every other shape takes the operations it took", [&] {
    expectOps("z = x *** p;", {"mul_plain"}, {"mul_plain"}, {2, 4, 6, 8});
    expectOps("z = x *** p +++ u;", {"mul_plain", "add"}, {"mul_plain", "add"}, {4, 6, 9, 11});
    expectOps("z = x *** 3 +++ y *** q;", two, two, {33, 6, 39, 212});  // a literal is no declared variable
    expectOps("z = x *** p +++ y *** q *** p;", {"mul_plain", "mul_plain", "mul_plain", "add"}, {"mul_plain", "mul_plain", "mul_plain", "add"},
              {62, 4, 66, 408});
    expectOps("z = x *** p --- y *** q;", {"mul_plain", "mul_plain", "sub"}, {"mul_plain", "mul_plain", "sub"}, {-28, 4, -24, -192});
    expectOps("z = u +++ x *** p +++ y *** q;", {"mul_plain", "add", "mul_plain", "add"}, {"mul_plain", "add", "mul_plain", "add"},
              {34, 6, 39, 211});  // not at the head of the sum
    expectOps("z = (x) *** p +++ y *** q;", two, two, {32, 4, 36, 208});
    expectOps("z = x *** y +++ y *** q;", {"mul", "mul_plain", "add"}, {"mul", "mul_plain", "add"}, {40, 40, 120, 360});  // a ciphertext product leads
  });
  t.run("the cleartext backend: no interface, same values", [] {
    DummyCiphertextFactory f;
    auto c = f.createCiphertext(std::vector<int64_t>{1, 2, 3});
    EXPECT_TRUE(dynamic_cast<PlainSumCapable *>(c.get()) == nullptr);
    CircuitRuntime rt(f, INPUTS);
    rt.executeAst("z = x *** p +++ q *** y +++ u *** p;");
    auto out = rt.getOutput("r = z;");
    std::vector<int64_t> z;
    f.decryptCiphertext(dynamic_cast<AbstractCiphertext &>(*out.at(0).second), z);
    z.resize(4);
    EXPECT_TRUE((z == std::vector<int64_t>{36, 8, 42, 214}));
    EXPECT_TRUE(run(FuseOn, "z = x *** p +++ q *** y +++ u *** p;").z == z);
  });
  return t.summary();
}
