// PlainSumCapable -- optional extension of a ciphertext: a sum of products of ciphertexts with public values, as one operation.
// Dot products with cleartext weights, box blurs and matrix-vector products by diagonals are sums `x *** p +++ y *** q (+++ ...)`.
// HipCiphertext implements it over abc_hip_bfv_multiply_plain_sum on BFV, where the one call gives the WORDS of multiplyPlain per
// term and addInplace (one inverse transform instead of one per product, the public values transformed once and cached); under CKKS
// multiplyPlain rescales per product, so words would change: it answers fusePlainSum() == false unless the factory's lazyRescale asks
// for exactly that trade (one abc_hip_multiply_plain_sum_rescale: the same values, one rescale rounding).  CircuitRuntime::additive uses
// the interface when the first ciphertext of a run offers it and fusePlainSum() says so.
// Not part of the reference's plugin surface: a ciphertext without it (DummyCiphertext) gets multiplyPlain and add_inplace per term,
// as upstream issues them.
#pragma once

#include <memory>
#include <utility>
#include <vector>

class AbstractCiphertext;
class ICleartext;

class PlainSumCapable {
 public:
  using Terms = std::vector<std::pair<const AbstractCiphertext *, const ICleartext *>>;
  virtual ~PlainSumCapable() = default;
  // the backend's option (HipSchemeConfig::fusePlainSum; under CKKS also lazyRescale); false: the interpreter issues what it always issued
  virtual bool fusePlainSum() const = 0;
  // sum over k of terms[k].first * terms[k].second, two terms or more, in the order written, terms[0].first == this: the value
  // multiplyPlain per term and addInplace give, with the same checks and exceptions
  virtual std::unique_ptr<AbstractCiphertext> plainSum(const Terms &terms) const = 0;
};
