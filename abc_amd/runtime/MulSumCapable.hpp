// MulSumCapable -- optional extension of a ciphertext: a sum of ciphertext products, relinearised ONCE, as one operation.
// Inner products over ciphertext lists, L2 distances, ciphertext-by-ciphertext matrix products and the cross terms of a polynomial
// evaluation are sums `x *** y +++ u *** v (+++ ...)`; relinearising the sum instead of every product saves all but one key switch
// and all but one round of key-switch noise (lazy relinearisation).  HipCiphertext implements it over abc_hip_mul_sum_relin;
// CircuitRuntime::additive uses it when the first factor offers it AND the backend asks for it (lazyRelinearize): the result
// decrypts to the same values, but its words differ from those of the per-product sequence, so a backend switches it on deliberately.
// Not part of the reference's plugin surface: a ciphertext without it (DummyCiphertext) gets multiply and add_inplace per term, as
// upstream issues them.
#pragma once

#include <memory>
#include <utility>
#include <vector>

class AbstractCiphertext;

class MulSumCapable {
 public:
  using Terms = std::vector<std::pair<const AbstractCiphertext *, const AbstractCiphertext *>>;
  virtual ~MulSumCapable() = default;
  // the backend's option (HipSchemeConfig::lazyRelinearize); off: the interpreter issues what it always issued
  virtual bool lazyRelinearize() const = 0;
  // sum over k of terms[k].first * terms[k].second, two terms or more, terms[0].first == this: decrypts to what
  // multiply per term and addInplace decrypt to, with the same checks and exceptions
  virtual std::unique_ptr<AbstractCiphertext> mulSum(const Terms &terms) const = 0;
};
