// CkksEncoder.hpp rounds ties away from zero, as abc_hip_ckks_encode and abc_hip_ckks_const_words do (include/abc_hip.h).  A constant
// slot vector c makes every butterfly sum of the transform exact, so coefficient 0 is exactly c * scale and every other coefficient
// zero: a tie the encoder can be held to.  (Its interface takes real slots only, so the coefficient N/2 pattern of
// tests/test_ckks_encoder.py, slots +-i c, has no counterpart here.)  Host only: no GPU, no libabc_hip.so.
#include <cmath>
#include <string>
#include <vector>

#include "CkksEncoder.hpp"
#include "mini_test.hpp"

int main() {
  MiniTest t;
  struct Tie {
    double value, scale;
    int64_t want;
  };
  const std::vector<Tie> ties = {{0.5, 1.0, 1},   {-0.5, 1.0, -1}, {1.5, 1.0, 2}, {2.5, 1.0, 3}, {-2.5, 1.0, -3}, {0x1p40 + 0.5, 1.0, (1ll << 40) + 1},
                                 {0x1p-41, 0x1p40, 1}, {0.49999999999999994, 1.0, 0}, {-0.49999999999999994, 1.0, 0}};
  const std::vector<uint64_t> primes = {1152921504606830593ull, 1099511480321ull};  // residues only: any moduli do
  for (size_t n : {(size_t)1024, (size_t)32768}) {
    CkksEncoder enc(n, primes);
    for (const Tie &tie : ties) {
      const std::string name = "N=" + std::to_string(n) + " constant " + std::to_string(tie.value) + " at scale " + std::to_string(tie.scale);
      t.run(name.c_str(), [&] {
        std::vector<uint64_t> out(primes.size() * n, ~0ull);
        enc.encode(std::vector<double>(n / 2, tie.value), tie.scale, (int)primes.size(), out.data());
        for (size_t j = 0; j < primes.size(); ++j) {
          const uint64_t q = primes[j], mag = (uint64_t)std::llabs(tie.want) % q;
          const uint64_t want = tie.want < 0 && mag ? q - mag : mag;
          if (out[j * n] != want)
            throw std::runtime_error("limb " + std::to_string(j) + ": coefficient 0 is " + std::to_string(out[j * n]) + ", want " + std::to_string(want));
          for (size_t k = 1; k < n; ++k)
            if (out[j * n + k]) throw std::runtime_error("limb " + std::to_string(j) + ": coefficient " + std::to_string(k) + " is not zero");
        }
      });
    }
  }
  return t.summary();
}
