// CircuitRuntime::additive's peephole on a recording fake backend: `lhs +++ rotate(v, k)` / `lhs + rotate(v, k)` becomes ONE
// addRotatedInplace on a ciphertext that offers RotateAddCapable, and everything else -- other shapes, malformed rotate calls, a
// backend without the interface -- goes down the path it always took: same operations, same results, same exception texts.
#include <string>
#include <vector>

#include "CircuitRuntime.hpp"
#include "DummyCiphertextFactory.hpp"
#include "RotateAddCapable.hpp"
#include "mini_test.hpp"

namespace {
std::vector<std::string> opLog;  // what the backend was asked to do, in order

// a cleartext slot vector whose rows rotate cyclically; Fused: offers RotateAddCapable
template <bool Fused>
class FakeFactory;

class FakeBase : public AbstractCiphertext {
 protected:
  [[noreturn]] static void no(const char *what) { throw std::runtime_error(std::string("fake backend: ") + what); }
  static const std::vector<int64_t> &dataOf(const AbstractCiphertext &c) { return dynamic_cast<const FakeBase &>(c).values; }
  void zip(const AbstractCiphertext &o, int sign) {
    const auto &r = dataOf(o);
    if (r.size() != values.size()) no("sizes differ");
    for (size_t i = 0; i < values.size(); ++i) values[i] += sign * r[i];
  }
  std::vector<int64_t> rotated(int steps) const {
    const long n = (long)values.size();
    std::vector<int64_t> r(values.size());
    for (long i = 0; i < n; ++i) r[i] = values[(size_t)((((i + steps) % n) + n) % n)];
    return r;
  }
  virtual std::unique_ptr<FakeBase> copy() const = 0;

 public:
  std::vector<int64_t> values;
  explicit FakeBase(const std::reference_wrapper<const AbstractCiphertextFactory> f) : AbstractCiphertext(f) {}
  std::unique_ptr<AbstractCiphertext> multiply(const AbstractCiphertext &o) const override { auto r = copy(); r->multiplyInplace(o); return r; }
  void multiplyInplace(const AbstractCiphertext &o) override {
    opLog.push_back("mul");
    const auto &r = dataOf(o);
    for (size_t i = 0; i < values.size(); ++i) values[i] *= r[i];
  }
  std::unique_ptr<AbstractCiphertext> multiplyPlain(const ICleartext &) const override { no("multiplyPlain"); }
  void multiplyPlainInplace(const ICleartext &) override { no("multiplyPlainInplace"); }
  std::unique_ptr<AbstractCiphertext> add(const AbstractCiphertext &o) const override { auto r = copy(); r->addInplace(o); return r; }
  void addInplace(const AbstractCiphertext &o) override { opLog.push_back("add"); zip(o, 1); }
  std::unique_ptr<AbstractCiphertext> addPlain(const ICleartext &) const override { no("addPlain"); }
  void addPlainInplace(const ICleartext &) override { no("addPlainInplace"); }
  std::unique_ptr<AbstractCiphertext> subtract(const AbstractCiphertext &o) const override { auto r = copy(); r->subtractInplace(o); return r; }
  void subtractInplace(const AbstractCiphertext &o) override { opLog.push_back("sub"); zip(o, -1); }
  std::unique_ptr<AbstractCiphertext> subtractPlain(const ICleartext &) const override { no("subtractPlain"); }
  void subtractPlainInplace(const ICleartext &) override { no("subtractPlainInplace"); }
  std::unique_ptr<AbstractCiphertext> rotateRows(int steps) const override {
    opLog.push_back("rotate " + std::to_string(steps));
    auto r = copy();
    r->values = rotated(steps);
    return r;
  }
  void rotateRowsInplace(int steps) override { opLog.push_back("rotate " + std::to_string(steps)); values = rotated(steps); }
  std::unique_ptr<AbstractCiphertext> clone() const override { return copy(); }

  void add_inplace(const AbstractValue &o) override { addInplace(dynamic_cast<const AbstractCiphertext &>(o)); }
  void subtract_inplace(const AbstractValue &o) override { subtractInplace(dynamic_cast<const AbstractCiphertext &>(o)); }
  void multiply_inplace(const AbstractValue &o) override { multiplyInplace(dynamic_cast<const AbstractCiphertext &>(o)); }
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
class FusingFake : public FakeBase, public RotateAddCapable {
  std::unique_ptr<FakeBase> copy() const override { return std::make_unique<FusingFake>(*this); }

 public:
  using FakeBase::FakeBase;
  void addRotatedInplace(const AbstractCiphertext &src, int steps) override {
    opLog.push_back("add_rotated " + std::to_string(steps));
    const auto r = dynamic_cast<const FusingFake &>(src).rotated(steps);
    for (size_t i = 0; i < values.size(); ++i) values[i] += r[i];
  }
};

template <bool Fused>
class FakeFactory : public AbstractCiphertextFactory {
  using Ct = std::conditional_t<Fused, FusingFake, PlainFake>;

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

const char *INPUTS = "secret int x = {1, 2, 3, 4, 5, 6, 7, 8}; secret int y = {10, 20, 30, 40, 50, 60, 70, 80}; "
                     "secret int z = {2, 2, 2, 2, 3, 3, 3, 3}; int p = {1, 1, 1, 1, 1, 1, 1, 1};";

struct Outcome {
  std::vector<std::string> ops;
  std::vector<int64_t> x;
  std::string error;  // what() of the exception, if the program threw
};
template <bool Fused>
Outcome run(const std::string &program) {
  FakeFactory<Fused> f;
  CircuitRuntime rt(f, INPUTS);
  opLog.clear();
  Outcome o;
  try {
    rt.executeAst(program);
    auto out = rt.getOutput("r = x;");
    f.decryptCiphertext(dynamic_cast<AbstractCiphertext &>(*out.at(0).second), o.x);
  } catch (const std::exception &e) {
    o.error = e.what();
  }
  o.ops = opLog;
  return o;
}
using Ops = std::vector<std::string>;

// on the fusing backend the program issues `fused`, on the plain one `plain`; both give the same x
void expectOps(const std::string &program, const Ops &fused, const Ops &plain, const std::vector<int64_t> &x) {
  const Outcome a = run<true>(program), b = run<false>(program);
  if (!a.error.empty() || !b.error.empty()) throw std::runtime_error(program + " threw: " + a.error + " / " + b.error);
  auto join = [](const Ops &v) { std::string s; for (auto &e : v) s += "[" + e + "]"; return s; };
  if (a.ops != fused) throw std::runtime_error(program + " on the fusing backend issued " + join(a.ops) + ", want " + join(fused));
  if (b.ops != plain) throw std::runtime_error(program + " on the plain backend issued " + join(b.ops) + ", want " + join(plain));
  if (a.x != x || b.x != x) throw std::runtime_error(program + " gave " + vecToString(a.x) + " / " + vecToString(b.x) + ", want " + vecToString(x));
}
// both backends refuse the program with exactly this text, having issued the same operations
void expectError(const std::string &program, const std::string &text) {
  const Outcome a = run<true>(program), b = run<false>(program);
  if (a.error != text || b.error != text)
    throw std::runtime_error(program + ": got \"" + a.error + "\" / \"" + b.error + "\", want \"" + text + "\"");
  if (a.ops != b.ops) throw std::runtime_error(program + ": the two backends issued different operations before the error");
}
}  // namespace

int main() {
  MiniTest t;
  t.run("x +++ rotate(v, k) is one fused call", [] {
    expectOps("x = x +++ rotate(x, 4);", {"add_rotated 4"}, {"rotate 4", "add"}, {6, 8, 10, 12, 6, 8, 10, 12});
    expectOps("x = x +++ rotate(y, -3);", {"add_rotated -3"}, {"rotate -3", "add"}, {61, 72, 83, 14, 25, 36, 47, 58});
    expectOps("x = x + rotate(y, 1);", {"add_rotated 1"}, {"rotate 1", "add"}, {21, 32, 43, 54, 65, 76, 87, 18});
    expectOps("x = x +++ rotate(y, 0);", {"add_rotated 0"}, {"rotate 0", "add"}, {11, 22, 33, 44, 55, 66, 77, 88});
    // a tree, and a sum of two rotations: every pair fuses
    expectOps("x = x +++ rotate(x, 4); x = x +++ rotate(x, 2); x = x +++ rotate(x, 1);", {"add_rotated 4", "add_rotated 2", "add_rotated 1"},
              {"rotate 4", "add", "rotate 2", "add", "rotate 1", "add"}, {36, 36, 36, 36, 36, 36, 36, 36});
    expectOps("x = x +++ rotate(y, 1) +++ rotate(y, -1);", {"add_rotated 1", "add_rotated -1"}, {"rotate 1", "add", "rotate -1", "add"},
              {101, 42, 63, 84, 105, 126, 147, 88});
    expectOps("x = (x +++ y) +++ rotate(z, 4);", {"add", "add_rotated 4"}, {"add", "rotate 4", "add"}, {14, 25, 36, 47, 57, 68, 79, 90});
  });
  t.run("every other shape takes the two operations", [] {
    expectOps("x = rotate(x, 1) +++ x;", {"rotate 1", "add"}, {"rotate 1", "add"}, {3, 5, 7, 9, 11, 13, 15, 9});
    expectOps("x = x +++ rotate(y, 2) *** z;", {"rotate 2", "mul", "add"}, {"rotate 2", "mul", "add"}, {61, 82, 103, 124, 215, 246, 37, 68});
    expectOps("x = x --- rotate(y, 1);", {"rotate 1", "sub"}, {"rotate 1", "sub"}, {-19, -28, -37, -46, -55, -64, -73, -2});
    expectOps("x = x +++ (rotate(y, 1));", {"rotate 1", "add"}, {"rotate 1", "add"}, {21, 32, 43, 54, 65, 76, 87, 18});
    expectOps("x = rotate(x, 4);", {"rotate 4"}, {"rotate 4"}, {5, 6, 7, 8, 1, 2, 3, 4});
    expectOps("x = x *** rotate(y, 0);", {"rotate 0", "mul"}, {"rotate 0", "mul"}, {10, 40, 90, 160, 250, 360, 490, 640});
  });
  t.run("malformed rotate calls keep their exception texts", [] {
    const std::string var = "Argument 'ciphertext' in 'rotate' instruction must be a variable.";
    const std::string steps = "Argument 'steps' in 'rotate' instruction must be an integer.";
    expectError("x = x +++ rotate(x +++ x, 2);", var);
    expectError("secret int r = rotate(x +++ x, 2);", var);
    expectError("x = x +++ rotate(4, 2);", var);
    expectError("x = x +++ rotate(x);", var);
    expectError("x = x +++ rotate(x, y);", steps);
    expectError("x = x +++ rotate(x, 1 + 1);", steps);
    expectError("x = x +++ rotate(x, -y);", steps);
    expectError("x = x +++ rotate(x, 2, 3);", steps);
    expectError("x = x +++ rotate(q, 1);", "rotate: 'q' is not a declared ciphertext.");
    expectError("x = x +++ rotate(p, 1);", "rotate: 'p' is not a declared ciphertext.");
    expectError("x = x +++ rotate(x, 1;", steps);
    expectError("x = x +++ turn(x, 1);", "Calls other than 'rotate(identifier: label, numSteps: int);' are not supported yet!");
    expectError("x = x +++ rotate;", "Parse error: expected '(' but found ';'.");
  });
  t.run("the cleartext backend does not offer the interface", [] {
    DummyCiphertextFactory f;
    auto c = f.createCiphertext(std::vector<int64_t>{1, 2, 3});
    EXPECT_TRUE(dynamic_cast<RotateAddCapable *>(c.get()) == nullptr);
    CircuitRuntime rt(f, "secret int a = {1, 2, 3};");
    std::string what;
    try { rt.executeAst("a = a +++ rotate(a, 1);"); } catch (const std::runtime_error &e) { what = e.what(); }
    EXPECT_TRUE(what == "Not yet implemented.");  // DummyCiphertext::rotateRows, as before
  });
  return t.summary();
}
