#include "HipCiphertext.hpp"

#include <algorithm>
#include <cmath>

#include "../../include/abc_hip.h"
#include "HipCiphertextFactory.hpp"

void abcHipCheck(int status, const char *what) {
  if (status != 0) throw std::runtime_error(std::string(what) + ": " + abc_hip_last_error());
}

namespace {
const HipCiphertext &cast(const AbstractCiphertext &c) {
  if (auto p = dynamic_cast<const HipCiphertext *>(&c)) return *p;
  throw std::runtime_error("Cast of AbstractCiphertext to HipCiphertext failed!");
}
const Cleartext<int> &intCleartext(const ICleartext &operand, const char *op) {
  if (auto p = dynamic_cast<const Cleartext<int> *>(&operand)) return *p;
  throw std::runtime_error(std::string(op) + "(Ciphertext,Cleartext) requires a Cleartext<int> as BFV supports integers only.");
}
struct DevicePlain {  // encoded plain operand, from the factory's cache (the reference re-encodes it on every plain op)
  const uint64_t *p;
  DevicePlain(const HipCiphertextFactory &fac, const std::vector<int> &v) : p(fac.cachedPlaintext(v)) {}
};
// CKKS plain operand: integer or real cleartexts
std::vector<double> realCleartext(const ICleartext &operand, const char *op) {
  if (auto p = dynamic_cast<const Cleartext<int> *>(&operand)) return std::vector<double>(p->getData().begin(), p->getData().end());
  if (auto p = dynamic_cast<const Cleartext<double> *>(&operand)) return p->getData();
  if (auto p = dynamic_cast<const Cleartext<float> *>(&operand)) return std::vector<double>(p->getData().begin(), p->getData().end());
  throw std::runtime_error(std::string(op) + "(Ciphertext,Cleartext) requires a Cleartext<int>, <float> or <double> under CKKS.");
}
// the one number a public value stands for: every entry equal (the factory pads a short vector with its last entry), and no more
// entries than the encoded path accepts (expandVector throws beyond `slots`: that vector stays with it, and is refused there)
bool oneNumber(const std::vector<double> &vals, size_t slots, double &c) {
  if (vals.empty() || vals.size() > slots) return false;
  for (double v : vals)
    if (!(v == vals[0])) return false;
  c = vals[0];
  return true;
}
}  // namespace

HipCiphertext::Buffer::~Buffer() {
  if (p) abc_hip_free(f.context(), p);  // stream-ordered: every use of the buffer was issued before this point
}

std::shared_ptr<HipCiphertext::Buffer> HipCiphertext::allocate(const HipCiphertextFactory &f, int level) {
  void *p = nullptr;
  abcHipCheck(abc_hip_malloc(f.context(), &p, f.ciphertextWords(level) * 8), "ciphertext allocation");
  return std::make_shared<Buffer>(f, static_cast<uint64_t *>(p));
}

HipCiphertext::HipCiphertext(const std::reference_wrapper<const HipCiphertextFactory> hipFactory)
    : AbstractCiphertext((const std::reference_wrapper<const AbstractCiphertextFactory>)hipFactory),
      buf(allocate(hipFactory.get(), hipFactory.get().dataLimbs())), nl(hipFactory.get().dataLimbs()),
      sc(hipFactory.get().isCkks() ? hipFactory.get().defaultScale() : 1.0) {}

HipCiphertext::HipCiphertext(const std::reference_wrapper<const HipCiphertextFactory> hipFactory, int level, double scale)
    : AbstractCiphertext((const std::reference_wrapper<const AbstractCiphertextFactory>)hipFactory),
      buf(allocate(hipFactory.get(), level)), nl(level), sc(scale) {
  if (level < 1 || level > hipFactory.get().dataLimbs()) throw std::runtime_error("HipCiphertext: level out of range");
}

HipCiphertext::~HipCiphertext() = default;

// "deep copy" by value semantics: shares the buffer until one side writes
HipCiphertext::HipCiphertext(const HipCiphertext &other) : AbstractCiphertext(other.factory), buf(other.buf), nl(other.nl), sc(other.sc) {}

HipCiphertext::HipCiphertext(HipCiphertext &&other) noexcept
    : AbstractCiphertext(other.factory), buf(std::move(other.buf)), nl(other.nl), sc(other.sc) {}

HipCiphertext &HipCiphertext::operator=(const HipCiphertext &other) { return *this = HipCiphertext(other); }

HipCiphertext &HipCiphertext::operator=(HipCiphertext &&other) {
  if (&other == this) return *this;
  if (&factory.get() != &other.factory.get())
    throw std::runtime_error("Cannot move Ciphertext from factory A into Ciphertext created by Factory B.");
  buf = std::move(other.buf);
  nl = other.nl;
  sc = other.sc;
  return *this;
}

std::shared_ptr<HipCiphertext::Buffer> HipCiphertext::target() const {
  return buf.use_count() == 1 ? buf : allocate(getFactory(), nl);
}

uint64_t *HipCiphertext::devicePtr() {
  if (buf.use_count() != 1) {  // a writer gets its own copy
    auto t = allocate(getFactory(), nl);
    abcHipCheck(abc_hip_memcpy_d2d(getFactory().context(), t->p, buf->p, getFactory().ciphertextWords(nl) * 8), "clone");
    buf = std::move(t);
  }
  return buf->p;
}

// ---- CKKS level / scale management ----
void HipCiphertext::dropTo(int level) {
  const auto &f = getFactory();
  while (nl > level) {  // Evaluator::mod_switch_to_next: CKKS simply drops the last limb
    auto t = allocate(f, nl - 1);
    abcHipCheck(abc_hip_mod_switch(f.context(), in(), t->p, 2, nl, f.batchSize()), "mod_switch");
    buf = std::move(t);
    --nl;
  }
}
void HipCiphertext::rescaleIfPossible() {
  const auto &f = getFactory();
  if (nl < 2) return;  // nothing left to divide by: the scale stays squared (documented in INTEGRATION.md)
  auto t = allocate(f, nl - 1);
  abcHipCheck(abc_hip_rescale(f.context(), in(), t->p, 2, nl, f.batchSize()), "rescale");
  sc /= (double)f.prime(nl - 1);
  buf = std::move(t);
  --nl;
}
bool HipCiphertext::scalesAgree(double a, double b) const {
  // written so that a NaN or a non-positive scale does not agree with anything
  const double rel = std::fabs(a - b) / std::fmax(std::fabs(a), std::fabs(b));
  return a > 0.0 && b > 0.0 && rel <= getFactory().scaleTolerance();
}
void HipCiphertext::checkScales(double a, double b) const {
  // after a rescale the scale is Delta^2 / q_l, a hair off Delta for a 40-bit prime next to Delta = 2^40, and that drift doubles
  // with every further squaring: adding values from different depths is what every CKKS program does (SEAL makes the user
  // overwrite the scale; here the left operand's scale stands).  The factory derives the bound from its chain
  // (HipCiphertextFactory::scaleTolerance); anything coarser is a real mismatch.  Written so that a NaN or a non-positive scale
  // fails too.
  if (!scalesAgree(a, b))
    throw std::runtime_error("CKKS: scale mismatch between operands (" + std::to_string(a) + " vs " + std::to_string(b) + ")");
}
// a product's scale must leave room under the modulus of its level, or the message wraps around silently (SEAL throws
// "scale out of bounds" at the same point)
void HipCiphertext::checkScaleFits(double scale, int level) const {
  const auto &f = getFactory();
  double bits = 0.0;
  for (int j = 0; j < level; ++j) bits += std::log2((double)f.prime(j));
  if (!std::isfinite(scale) || !(scale > 0.0) || !(std::log2(scale) < bits - 1.0))
    throw std::runtime_error("CKKS: scale 2^" + std::to_string(std::log2(scale)) + " out of bounds for a modulus of " + std::to_string(bits) +
                             " bits (no limb left to rescale into)");
}
const uint64_t *HipCiphertext::alignWith(const HipCiphertext &operand, std::shared_ptr<Buffer> &keep) {
  const auto &f = getFactory();
  if (!f.isCkks() || operand.nl == nl) return operand.in();
  if (operand.nl < nl) {  // we are the one to come down
    dropTo(operand.nl);
    return operand.in();
  }
  // the operand is const: bring a temporary copy of it down to our level
  const uint64_t *src = operand.in();
  for (int l = operand.nl; l > nl; --l) {
    auto t = allocate(f, l - 1);
    abcHipCheck(abc_hip_mod_switch(f.context(), src, t->p, 2, l, f.batchSize()), "mod_switch");
    keep = std::move(t);
    src = keep->p;
  }
  return src;
}

const HipCiphertextFactory &HipCiphertext::getFactory() const {
  if (auto f = dynamic_cast<const HipCiphertextFactory *>(&factory.get())) return *f;
  throw std::runtime_error("Cast of AbstractFactory to HipFactory failed. HipCiphertext is probably invalid.");
}

std::unique_ptr<HipCiphertext> HipCiphertext::fresh(int level) const {
  auto r = std::make_unique<HipCiphertext>(*this);  // same factory, level and scale bookkeeping
  r->buf = allocate(getFactory(), level);
  r->nl = level;
  return r;
}
std::unique_ptr<HipCiphertext> HipCiphertext::clone_impl() const { return std::make_unique<HipCiphertext>(*this); }
std::unique_ptr<AbstractCiphertext> HipCiphertext::clone() const { return clone_impl(); }

std::vector<int> HipCiphertext::noiseBitsBatch() const {
  const auto &f = getFactory();
  if (f.isCkks()) throw std::runtime_error("noiseBits: the invariant noise budget is defined for BFV only; this factory runs CKKS.");
  std::vector<int> bits(f.batchSize());
  abcHipCheck(abc_hip_noise_budget(f.context(), in(), 2, nl, bits.data(), bits.size()), "noise_budget");
  return bits;
}
int HipCiphertext::noiseBits() const {
  const std::vector<int> bits = noiseBitsBatch();
  return *std::min_element(bits.begin(), bits.end());
}

// ---- ctxt-ctxt ----
// returning forms = copy-on-write clone + in-place form (a clone is a reference; the in-place form on a shared buffer
// computes out of place into a fresh one, so no device-to-device copy is made either way)
std::unique_ptr<AbstractCiphertext> HipCiphertext::add(const AbstractCiphertext &operand) const {
  auto r = clone_impl();
  r->addInplace(operand);
  return r;
}
std::unique_ptr<AbstractCiphertext> HipCiphertext::subtract(const AbstractCiphertext &operand) const {
  auto r = clone_impl();
  r->subtractInplace(operand);
  return r;
}
std::unique_ptr<AbstractCiphertext> HipCiphertext::multiply(const AbstractCiphertext &operand) const {
  auto r = clone_impl();
  r->multiplyInplace(operand);
  return r;
}
void HipCiphertext::addInplace(const AbstractCiphertext &operand) {
  std::shared_ptr<Buffer> keep;
  const uint64_t *rhs = alignWith(cast(operand), keep);
  if (getFactory().isCkks()) checkScales(sc, cast(operand).sc);
  auto t = target();
  abcHipCheck(abc_hip_add(getFactory().context(), in(), rhs, t->p, 2, nl, getFactory().batchSize()), "add");
  adopt(std::move(t));
}
void HipCiphertext::subtractInplace(const AbstractCiphertext &operand) {
  std::shared_ptr<Buffer> keep;
  const uint64_t *rhs = alignWith(cast(operand), keep);
  if (getFactory().isCkks()) checkScales(sc, cast(operand).sc);
  auto t = target();
  abcHipCheck(abc_hip_sub(getFactory().context(), in(), rhs, t->p, 2, nl, getFactory().batchSize()), "sub");
  adopt(std::move(t));
}
void HipCiphertext::multiplyInplace(const AbstractCiphertext &operand) {
  // Evaluator::multiply + relinearize_inplace, src/runtime/SealCiphertext.cpp:102-107 (CKKS: + rescale_to_next)
  std::shared_ptr<Buffer> keep;
  const uint64_t *rhs = alignWith(cast(operand), keep);
  auto t = target();
  abcHipCheck(abc_hip_mul_relin(getFactory().context(), in(), rhs, t->p, nl, getFactory().batchSize()), "multiply");
  adopt(std::move(t));
  if (getFactory().isCkks()) {
    sc *= cast(operand).sc;
    checkScaleFits(sc, nl);
    rescaleIfPossible();
  }
}

// ---- rotation ----
std::unique_ptr<AbstractCiphertext> HipCiphertext::rotateRows(int steps) const {
  auto r = fresh(nl);
  abcHipCheck(abc_hip_rotate(getFactory().context(), in(), r->buf->p, nl, steps, getFactory().batchSize()), "rotate_rows");
  return r;
}
void HipCiphertext::rotateRowsInplace(int steps) {
  auto t = target();
  abcHipCheck(abc_hip_rotate(getFactory().context(), in(), t->p, nl, steps, getFactory().batchSize()), "rotate_rows");
  adopt(std::move(t));
}

void HipCiphertext::addRotatedInplace(const AbstractCiphertext &src, int steps) {
  const HipCiphertext &s = cast(src);
  const auto &f = getFactory();
  if (!f.fusesRotateAdd() || s.nl != nl) {  // the two calls: they also bring operands at different levels together
    auto r = s.rotateRows(steps);
    addInplace(*r);
    return;
  }
  if (f.isCkks()) checkScales(sc, s.sc);
  auto t = allocate(f, nl);  // never the own buffer: `x +++ rotate(x, k)` would rotate in place, which no key switch gathers from
  abcHipCheck(abc_hip_rotate_add(f.context(), s.in(), in(), t->p, nl, steps, f.batchSize()), "rotate_add");
  f.countFusedRotateAdd();
  adopt(std::move(t));
}

bool HipCiphertext::lazyRelinearize() const { return getFactory().lazyRelinearizes(); }

std::unique_ptr<AbstractCiphertext> HipCiphertext::mulSum(const MulSumCapable::Terms &terms) const {
  const auto &f = getFactory();
  bool one_level = !terms.empty();
  for (const auto &t : terms) one_level = one_level && cast(*t.first).nl == nl && cast(*t.second).nl == nl;
  if (!one_level || !f.lazyRelinearizes()) {  // the calls per term: they also bring operands at different levels together
    if (terms.empty()) throw std::runtime_error("mulSum: no terms");
    auto r = terms[0].first->multiply(*terms[0].second);
    for (size_t k = 1; k < terms.size(); ++k) r->addInplace(*terms[k].first->multiply(*terms[k].second));
    return r;
  }
  const double scale = f.isCkks() ? cast(*terms[0].first).sc * cast(*terms[0].second).sc : 1.0;
  std::vector<const uint64_t *> a, b;
  for (const auto &t : terms) {
    if (f.isCkks()) checkScales(scale, cast(*t.first).sc * cast(*t.second).sc);
    a.push_back(cast(*t.first).in());
    b.push_back(cast(*t.second).in());
  }
  auto r = fresh(nl);
  abcHipCheck(abc_hip_mul_sum_relin(f.context(), a.data(), b.data(), (int)terms.size(), r->buf->p, nl, f.batchSize()), "mul_sum_relin");
  f.countMulSum();
  if (f.isCkks()) {
    r->sc = scale;
    r->checkScaleFits(r->sc, r->nl);
    r->rescaleIfPossible();
  }
  return r;
}

bool HipCiphertext::fusePlainSum() const {
  const auto &f = getFactory();
  return f.fusesPlainSum() && (!f.isCkks() || f.lazyRescales());
}

// CKKS: one abc_hip_multiply_plain_sum_rescale where every term sits at this level (two limbs or more) and scale and no public value is
// all -1; else null, and the caller takes the calls per term.  Runs longer than the plaintext cache go in slices: the leading ones
// by abc_hip_multiply_plain_sum at nl with the sum so far as addend, the last one by the new call with that sum as its addend.
// `held` keeps every block of a slice alive until its call is enqueued, whatever a later miss of the same slice evicts.
std::unique_ptr<HipCiphertext> HipCiphertext::ckksPlainSumRescale(const PlainSumCapable::Terms &terms) const {
  const auto &f = getFactory();
  if (!fusePlainSum() || nl < 2) return nullptr;
  std::vector<std::vector<double>> vals;
  for (const auto &t : terms) {
    const HipCiphertext &c = cast(*t.first);
    vals.push_back(realCleartext(*t.second, "MULTIPLY"));
    bool allMinusOne = !vals.back().empty();
    for (double v : vals.back()) allMinusOne = allMinusOne && v == -1.0;
    if (allMinusOne || c.nl != nl || !scalesAgree(sc, c.sc)) return nullptr;
  }
  const double ps = f.defaultScale();
  checkScaleFits(sc * ps, nl);  // throws before anything is enqueued
  std::shared_ptr<Buffer> sum;  // the leading slices' sum, nl limbs
  std::unique_ptr<HipCiphertext> r;
  for (size_t k0 = 0; k0 < terms.size(); k0 += f.plainCacheEntries()) {
    const size_t k1 = std::min(terms.size(), k0 + f.plainCacheEntries());
    std::vector<const uint64_t *> a, p;
    std::vector<std::shared_ptr<const HipCiphertextFactory::DeviceBlock>> held;
    for (size_t k = k0; k < k1; ++k) {
      a.push_back(cast(*terms[k].first).in());
      held.push_back(f.cachedCkksPlaintextBlock(vals[k], nl, ps));
      p.push_back(held.back()->p);
    }
    if (k1 < terms.size()) {
      const uint64_t *addend = sum ? sum->p : nullptr;
      if (!sum) sum = allocate(f, nl);
      abcHipCheck(abc_hip_multiply_plain_sum(f.context(), a.data(), p.data(), 0, (int)a.size(), addend, sum->p, 2, nl, f.batchSize()), "multiply_plain_sum");
    } else {
      r = fresh(nl - 1);
      abcHipCheck(abc_hip_multiply_plain_sum_rescale(f.context(), a.data(), p.data(), 0, (int)a.size(), sum ? sum->p : nullptr, r->buf->p, 2, nl,
                                                     f.batchSize()),
                  "multiply_plain_sum_rescale");
      f.countPlainSumRescale();
    }
  }
  r->sc = sc * ps / (double)f.prime(nl - 1);
  return r;
}

std::unique_ptr<AbstractCiphertext> HipCiphertext::plainSum(const PlainSumCapable::Terms &terms) const {
  const auto &f = getFactory();
  if (terms.empty()) throw std::runtime_error("plainSum: no terms");
  if (f.isCkks()) {
    if (auto r = ckksPlainSumRescale(terms)) return r;
    auto r = terms[0].first->multiplyPlain(*terms[0].second);  // the calls per term, as the interpreter issues them
    for (size_t k = 1; k < terms.size(); ++k) r->addInplace(*terms[k].first->multiplyPlain(*terms[k].second));
    return r;
  }
  bool one_call = fusePlainSum();
  for (const auto &t : terms) {
    if (!one_call) break;
    one_call = !intCleartext(*t.second, "MULTIPLY").allEqual(-1) && cast(*t.first).nl == nl;  // -1: multiplyPlain negates instead
  }
  if (!one_call) {  // the calls per term, as the interpreter issues them
    auto r = terms[0].first->multiplyPlain(*terms[0].second);
    for (size_t k = 1; k < terms.size(); ++k) r->addInplace(*terms[k].first->multiplyPlain(*terms[k].second));
    return r;
  }
  // at most plainCacheEntries() terms per call, so that a slice's plaintexts fit the cache together; `held` keeps every block of the
  // slice alive until the call is enqueued, whatever a later miss of the same slice evicts (a hit on the oldest entry followed by a
  // miss on a full cache would otherwise free the block just gathered).  A later slice takes the sum so far as its addend
  auto r = fresh(nl);
  for (size_t k0 = 0; k0 < terms.size(); k0 += f.plainCacheEntries()) {
    const size_t k1 = std::min(terms.size(), k0 + f.plainCacheEntries());
    std::vector<const uint64_t *> a, p;
    std::vector<std::shared_ptr<const HipCiphertextFactory::DeviceBlock>> held;
    for (size_t k = k0; k < k1; ++k) {
      a.push_back(cast(*terms[k].first).in());
      held.push_back(f.cachedPlaintextNtt(intCleartext(*terms[k].second, "MULTIPLY").getData()));
      p.push_back(held.back()->p);
    }
    abcHipCheck(abc_hip_bfv_multiply_plain_sum(f.context(), a.data(), ABC_HIP_CT_COEFF, p.data(), 0, (int)a.size(), k0 ? r->buf->p : nullptr,
                                               r->buf->p, 2, f.batchSize()),
                "bfv_multiply_plain_sum");
    f.countPlainSum();
  }
  return r;
}

// ---- ctxt-plain ----
std::unique_ptr<AbstractCiphertext> HipCiphertext::addPlain(const ICleartext &operand) const {
  auto r = clone_impl();
  r->addPlainInplace(operand);
  return r;
}
std::unique_ptr<AbstractCiphertext> HipCiphertext::subtractPlain(const ICleartext &operand) const {
  auto r = clone_impl();
  r->subtractPlainInplace(operand);
  return r;
}
std::unique_ptr<AbstractCiphertext> HipCiphertext::multiplyPlain(const ICleartext &operand) const {
  auto r = clone_impl();
  r->multiplyPlainInplace(operand);
  return r;
}
// HipSchemeConfig::constOperands: this value plus the constant c at this value's own scale, the K = 0 form of
// abc_hip_multiply_const_sum (component 0 only); no plaintext, no cache entry
void HipCiphertext::addConstInplace(double c) {
  const auto &f = getFactory();
  uint64_t w[16];
  abcHipCheck(abc_hip_ckks_const_words(f.context(), c, sc, nl, w), "ckks_const_words");
  auto t = target();
  abcHipCheck(abc_hip_multiply_const_sum(f.context(), nullptr, nullptr, nullptr, 0, w, in(), t->p, 2, nl, f.batchSize()), "multiply_const_sum");
  f.countConstOperand();
  adopt(std::move(t));
}
void HipCiphertext::addPlainInplace(const ICleartext &operand) {
  if (getFactory().isCkks()) {  // encoded at this value's own level and scale: exact scale match
    double c;
    if (getFactory().takesConstOperands() && oneNumber(realCleartext(operand, "ADD"), getFactory().usableSlots(), c)) return addConstInplace(c);
    const uint64_t *pl = getFactory().cachedCkksPlaintext(realCleartext(operand, "ADD"), nl, sc);
    auto t = target();
    abcHipCheck(abc_hip_add_plain(getFactory().context(), in(), pl, 0, t->p, 2, nl, getFactory().batchSize()), "add_plain");
    adopt(std::move(t));
    return;
  }
  DevicePlain pl(getFactory(), intCleartext(operand, "ADD").getData());
  auto t = target();
  abcHipCheck(abc_hip_add_plain(getFactory().context(), in(), pl.p, 0, t->p, 2, nl, getFactory().batchSize()), "add_plain");
  adopt(std::move(t));
}
void HipCiphertext::subtractPlainInplace(const ICleartext &operand) {
  if (getFactory().isCkks()) {
    double c;
    if (getFactory().takesConstOperands() && oneNumber(realCleartext(operand, "SUB"), getFactory().usableSlots(), c)) return addConstInplace(-c);  // const_words(-c)
    const uint64_t *pl = getFactory().cachedCkksPlaintext(realCleartext(operand, "SUB"), nl, sc);
    auto t = target();
    abcHipCheck(abc_hip_sub_plain(getFactory().context(), in(), pl, 0, t->p, 2, nl, getFactory().batchSize()), "sub_plain");
    adopt(std::move(t));
    return;
  }
  DevicePlain pl(getFactory(), intCleartext(operand, "SUB").getData());
  auto t = target();
  abcHipCheck(abc_hip_sub_plain(getFactory().context(), in(), pl.p, 0, t->p, 2, nl, getFactory().batchSize()), "sub_plain");
  adopt(std::move(t));
}
void HipCiphertext::multiplyPlainInplace(const ICleartext &operand) {
  if (getFactory().isCkks()) {
    const auto vals = realCleartext(operand, "MULTIPLY");
    bool allMinusOne = !vals.empty();
    for (double v : vals) allMinusOne = allMinusOne && v == -1.0;
    if (allMinusOne) {  // negation shortcut, src/runtime/SealCiphertext.cpp:192-193: no level is spent
      auto t = target();
      abcHipCheck(abc_hip_negate(getFactory().context(), in(), t->p, 2, nl, getFactory().batchSize()), "negate");
      adopt(std::move(t));
      return;
    }
    const double ps = getFactory().defaultScale();
    double c;
    if (getFactory().takesConstOperands() && oneNumber(vals, getFactory().usableSlots(), c)) {
      // the scalar as per-limb words, at the scale the encoded path would have used: one abc_hip_multiply_const_sum_rescale where a
      // limb is left to drop (bookkeeping as below), the product alone at one limb; the checks throw before anything is enqueued
      const auto &f = getFactory();
      uint64_t w[16];
      abcHipCheck(abc_hip_ckks_const_words(f.context(), c, ps, nl, w), "ckks_const_words");
      checkScaleFits(sc * ps, nl);
      const uint64_t *term = in();
      if (nl >= 2) {
        auto r = allocate(f, nl - 1);
        abcHipCheck(abc_hip_multiply_const_sum_rescale(f.context(), &term, nullptr, w, 1, nullptr, nullptr, r->p, 2, nl, f.batchSize()), "multiply_const_sum_rescale");
        sc = sc * ps / (double)f.prime(nl - 1);
        buf = std::move(r);
        --nl;
      } else {
        auto t = allocate(f, nl);  // never in place: the sum's output may not be one of its terms
        abcHipCheck(abc_hip_multiply_const_sum(f.context(), &term, nullptr, w, 1, nullptr, nullptr, t->p, 2, nl, f.batchSize()), "multiply_const_sum");
        adopt(std::move(t));
        sc *= ps;
      }
      f.countConstOperand();
      return;
    }
    const uint64_t *pl = getFactory().cachedCkksPlaintext(vals, nl, ps);
    if (nl >= 2 && getFactory().fusesMultiplyPlainRescale()) {
      // product and rescale as one call: the words of the two calls below, bookkeeping as rescaleIfPossible does it; the check
      // throws before anything is enqueued
      const auto &f = getFactory();
      checkScaleFits(sc * ps, nl);
      auto r = allocate(f, nl - 1);
      abcHipCheck(abc_hip_multiply_plain_rescale(f.context(), in(), pl, 0, r->p, 2, nl, f.batchSize()), "multiply_plain_rescale");
      f.countFusedMultiplyPlainRescale();
      sc = sc * ps / (double)f.prime(nl - 1);
      buf = std::move(r);
      --nl;
      return;
    }
    auto t = target();
    abcHipCheck(abc_hip_multiply_plain(getFactory().context(), in(), pl, 0, t->p, 2, nl, getFactory().batchSize()), "multiply_plain");
    adopt(std::move(t));
    sc *= ps;
    checkScaleFits(sc, nl);
    rescaleIfPossible();
    return;
  }
  const auto &ct = intCleartext(operand, "MULTIPLY");
  if (ct.allEqual(-1)) {  // negation shortcut, src/runtime/SealCiphertext.cpp:192-193
    auto t = target();
    abcHipCheck(abc_hip_negate(getFactory().context(), in(), t->p, 2, nl, getFactory().batchSize()), "negate");
    adopt(std::move(t));
    return;
  }
  DevicePlain pl(getFactory(), ct.getData());
  // multiply_plain keeps size 2, so the reference's relinearize_inplace (:197) is a no-op
  auto t = target();
  abcHipCheck(abc_hip_multiply_plain(getFactory().context(), in(), pl.p, 0, t->p, 2, nl, getFactory().batchSize()),
              "multiply_plain");
  adopt(std::move(t));
}

// ---- AbstractValue dispatch (src/runtime/SealCiphertext.cpp:208-239) ----
void HipCiphertext::add_inplace(const AbstractValue &other) {
  if (auto c = dynamic_cast<const HipCiphertext *>(&other)) addInplace(*c);
  else if (auto p = dynamic_cast<const ICleartext *>(&other)) addPlainInplace(*p);
  else throw std::runtime_error("Operation ADD only supported for (AbstractCiphertext,AbstractCiphertext) and (HipCiphertext, ICleartext).");
}
void HipCiphertext::subtract_inplace(const AbstractValue &other) {
  if (auto c = dynamic_cast<const HipCiphertext *>(&other)) subtractInplace(*c);
  else if (auto p = dynamic_cast<const ICleartext *>(&other)) subtractPlainInplace(*p);
  else throw std::runtime_error("Operation SUBTRACT only supported for (HipCiphertext,HipCiphertext) and (HipCiphertext, ICleartext).");
}
void HipCiphertext::multiply_inplace(const AbstractValue &other) {
  if (auto c = dynamic_cast<const HipCiphertext *>(&other)) multiplyInplace(*c);
  else if (auto p = dynamic_cast<const ICleartext *>(&other)) multiplyPlainInplace(*p);
  else throw std::runtime_error("Operation MULTIPLY only supported for (HipCiphertext,HipCiphertext) and (HipCiphertext, ICleartext).");
}
#define ABC_UNSUPPORTED(name) \
  void HipCiphertext::name(const AbstractValue &) { throw std::runtime_error("Operation " #name " not supported for (HipCiphertext, ANY)."); }
ABC_UNSUPPORTED(divide_inplace)
ABC_UNSUPPORTED(modulo_inplace)
ABC_UNSUPPORTED(logicalAnd_inplace)
ABC_UNSUPPORTED(logicalOr_inplace)
ABC_UNSUPPORTED(logicalLess_inplace)
ABC_UNSUPPORTED(logicalLessEqual_inplace)
ABC_UNSUPPORTED(logicalGreater_inplace)
ABC_UNSUPPORTED(logicalGreaterEqual_inplace)
ABC_UNSUPPORTED(logicalEqual_inplace)
ABC_UNSUPPORTED(logicalNotEqual_inplace)
ABC_UNSUPPORTED(bitwiseAnd_inplace)
ABC_UNSUPPORTED(bitwiseXor_inplace)
ABC_UNSUPPORTED(bitwiseOr_inplace)
#undef ABC_UNSUPPORTED
void HipCiphertext::logicalNot_inplace() {
  throw std::runtime_error("Operation logicalNot_inplace not supported for (HipCiphertext, ANY). For an arithmetic negation, multiply_inplace by (-1) instead.");
}
void HipCiphertext::bitwiseNot_inplace() {
  throw std::runtime_error("Operation bitwiseNot_inplace not supported for (HipCiphertext, ANY). For an arithmetic negation, multiply_inplace by (-1) instead.");
}
