// RotateAddCapable -- optional extension of a ciphertext: `*this += rotate(src, steps)` as ONE operation.  Rotate-and-sum trees
// (`x = x +++ rotate(x, s);`, what CircuitVectorizer / ExpressionBatcher emit, and the reference's dot product, Hamming, L2,
// matrix-vector and box blur programs) are nothing but this pair; a backend whose key switch can take the addend as one more
// operand of its last kernel saves the rotated ciphertext's trip through memory and one call.  HipCiphertext implements it over
// abc_hip_rotate_add; CircuitRuntime::additive uses it when the left operand offers it.  Not part of the reference's plugin
// surface: a ciphertext without it (DummyCiphertext) gets rotateRows followed by add_inplace, as upstream issues them.
#pragma once

class AbstractCiphertext;

class RotateAddCapable {
 public:
  virtual ~RotateAddCapable() = default;
  // same result, same checks and same exceptions as `auto r = src.rotateRows(steps); this->addInplace(*r);`
  virtual void addRotatedInplace(const AbstractCiphertext &src, int steps) = 0;
};
