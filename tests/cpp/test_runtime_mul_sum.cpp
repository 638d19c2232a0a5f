// CircuitRuntime::additive's peephole for sums of products, on a recording fake backend: a run `x *** y +++ u *** v (+++ ...)` of two
// or more products of declared secret variables becomes ONE MulSumCapable::mulSum when the first factor offers the interface and the
// backend asks for lazy relinearisation; every other shape, a backend without the interface and one with the option off issue what
// they always issued.  The decoded values are the same either way, on the fakes and on the cleartext (Dummy) backend.
#include <string>
#include <vector>

#include "CircuitRuntime.hpp"
#include "DummyCiphertextFactory.hpp"
#include "MulSumCapable.hpp"
#include "mini_test.hpp"

namespace {
std::vector<std::string> opLog;  // what the backend was asked to do, in order
enum Mode { Plain, LazyOff, LazyOn };

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
class LazyFake : public FakeBase, public MulSumCapable {
  std::unique_ptr<FakeBase> copy() const override { return std::make_unique<LazyFake>(*this); }

 public:
  using FakeBase::FakeBase;
  bool lazyRelinearize() const override { return On; }
  std::unique_ptr<AbstractCiphertext> mulSum(const Terms &terms) const override {
    if (terms.empty() || terms[0].first != this) no("mulSum: the first factor is the receiver");
    opLog.push_back("mul_sum " + std::to_string(terms.size()));
    auto r = std::make_unique<LazyFake>(*this);
    for (auto &v : r->values) v = 0;
    for (const auto &t : terms)
      for (size_t i = 0; i < r->values.size(); ++i) r->values[i] += dataOf(*t.first)[i] * dataOf(*t.second)[i];
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
                     "secret int v = {5, 6, 7, 8}; secret int w = {1, 0, 1, 0}; secret int z = {0, 0, 0, 0}; int p = {2, 2, 2, 2};";

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
  if (m == LazyOn) { FakeFactory<LazyFake<true>> f; return runOn(f, program); }
  if (m == LazyOff) { FakeFactory<LazyFake<false>> f; return runOn(f, program); }
  FakeFactory<PlainFake> f;
  return runOn(f, program);
}
using Ops = std::vector<std::string>;

// with the interface offered and on the program issues `lazy`; offered but off, and not offered, `eager`; the same z everywhere
void expectOps(const std::string &program, const Ops &lazy, const Ops &eager, const std::vector<int64_t> &z) {
  auto join = [](const Ops &v) { std::string s; for (auto &e : v) s += "[" + e + "]"; return s; };
  for (Mode m : {LazyOn, LazyOff, Plain}) {
    const Outcome o = run(m, program);
    const Ops &want = m == LazyOn ? lazy : eager;
    if (o.ops != want) throw std::runtime_error(program + " in mode " + std::to_string(m) + " issued " + join(o.ops) + ", want " + join(want));
    if (o.z != z) throw std::runtime_error(program + " in mode " + std::to_string(m) + " gave " + vecToString(o.z) + ", want " + vecToString(z));
  }
}
}  // namespace

int main() {
  MiniTest t;
  t.run("a run of products is one mul_sum when offered and asked for", [] {
    expectOps("z = x *** y +++ u *** v;", {"mul_sum 2"}, {"mul", "mul", "add"}, {20, 52, 111, 184});
    expectOps("z = x * y + u * v;", {"mul_sum 2"}, {"mul", "mul", "add"}, {20, 52, 111, 184});
    expectOps("z = x *** y +++ u *** v +++ w *** x;", {"mul_sum 3"}, {"mul", "mul", "add", "mul", "add"}, {21, 52, 114, 184});
    expectOps("z = x *** x +++ y *** y;", {"mul_sum 2"}, {"mul", "mul", "add"}, {101, 404, 909, 1616});  // squares; one variable twice
    expectOps("secret int s = x *** y +++ u *** v; z = s;", {"mul_sum 2"}, {"mul", "mul", "add"}, {20, 52, 111, 184});
    // what follows the run is added, subtracted or compared as it always was
    expectOps("z = x *** y +++ u *** v +++ w;", {"mul_sum 2", "add"}, {"mul", "mul", "add", "add"}, {21, 52, 112, 184});
    expectOps("z = x *** y +++ u *** v --- w *** x;", {"mul_sum 2", "mul", "sub"}, {"mul", "mul", "add", "mul", "sub"}, {19, 52, 108, 184});
    expectOps("z = (x *** y +++ u *** v) *** w;", {"mul_sum 2", "mul"}, {"mul", "mul", "add", "mul"}, {20, 0, 111, 0});
    // a product that does not qualify ends the run in front of it
    expectOps("z = x *** y +++ u *** v +++ w *** x *** y;", {"mul_sum 2", "mul", "mul", "add"}, {"mul", "mul", "add", "mul", "mul", "add"},
              {30, 52, 201, 184});
  });
  t.run("every other shape takes the operations it took", [] {
    expectOps("z = x *** y +++ u;", {"mul", "add"}, {"mul", "add"}, {12, 42, 93, 163});
    expectOps("z = x *** y;", {"mul"}, {"mul"}, {10, 40, 90, 160});
    expectOps("z = x *** y +++ u *** v *** w;", {"mul", "mul", "mul", "add"}, {"mul", "mul", "mul", "add"}, {20, 40, 111, 160});
    expectOps("z = x *** 3 +++ u *** v;", {"mul_plain", "mul", "add"}, {"mul_plain", "mul", "add"}, {13, 18, 30, 36});
    expectOps("z = x *** p +++ u *** v;", {"mul_plain", "mul", "add"}, {"mul_plain", "mul", "add"}, {12, 16, 27, 32});  // a public factor
    expectOps("z = p *** x +++ u *** v;", {"mul_plain", "mul", "add"}, {"mul_plain", "mul", "add"}, {12, 16, 27, 32});
    expectOps("z = x *** y --- u *** v;", {"mul", "mul", "sub"}, {"mul", "mul", "sub"}, {0, 28, 69, 136});
    expectOps("z = u +++ x *** y +++ u *** v;", {"mul", "add", "mul", "add"}, {"mul", "add", "mul", "add"}, {22, 54, 114, 187});  // not at the head of the sum
    expectOps("z = (x) *** y +++ u *** v;", {"mul", "mul", "add"}, {"mul", "mul", "add"}, {20, 52, 111, 184});
  });
  t.run("the cleartext backend: no interface, same values", [] {
    DummyCiphertextFactory f;
    auto c = f.createCiphertext(std::vector<int64_t>{1, 2, 3});
    EXPECT_TRUE(dynamic_cast<MulSumCapable *>(c.get()) == nullptr);
    CircuitRuntime rt(f, INPUTS);
    rt.executeAst("z = x *** y +++ u *** v +++ w *** x;");
    auto out = rt.getOutput("r = z;");
    std::vector<int64_t> z;
    f.decryptCiphertext(dynamic_cast<AbstractCiphertext &>(*out.at(0).second), z);
    z.resize(4);
    EXPECT_TRUE((z == std::vector<int64_t>{21, 52, 114, 184}));
    EXPECT_TRUE(run(LazyOn, "z = x *** y +++ u *** v +++ w *** x;").z == z);
  });
  return t.summary();
}
