// Stand-alone driver of the keyed sampling spec's host twin (abc_amd/csrc/abc_sample.hpp), for tests/test_keyed_sampling_spec.py:
// plain C++ (no HIP, no GPU), so it builds with -fsanitize=address,undefined.
//   small <64 hex digits of key> <nonce> <n> <count>   the body of abc_hip_keyed_small_host: count*3*n int8, as decimal text
//   edge <lo> <hi> <q> ...                              per triple: ternary(lo) ternary(hi) uniform_q(lo, hi, q)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "abc_sample.hpp"

int main(int argc, char **argv) {
  if (argc >= 6 && !std::strcmp(argv[1], "small") && std::strlen(argv[2]) == 64) {
    uint8_t key[32];
    for (int i = 0; i < 32; i++) {
      unsigned v = 0;
      if (std::sscanf(argv[2] + 2 * i, "%2x", &v) != 1) return 2;
      key[i] = (uint8_t)v;
    }
    const uint64_t nonce = std::strtoull(argv[3], nullptr, 0);
    const size_t n = std::strtoull(argv[4], nullptr, 0), count = std::strtoull(argv[5], nullptr, 0);
    if (!n || n % 8) return 2;
    std::vector<int8_t> out(count * 3 * n);
    abc::keyed::encrypt_small_host(key, nonce, n, count, out.data());
    for (int8_t v : out) std::printf("%d\n", (int)v);
    return 0;
  }
  if (argc >= 5 && !std::strcmp(argv[1], "edge") && (argc - 2) % 3 == 0) {
    for (int i = 2; i < argc; i += 3) {
      const uint64_t lo = std::strtoull(argv[i], nullptr, 0), hi = std::strtoull(argv[i + 1], nullptr, 0);
      const uint64_t q = std::strtoull(argv[i + 2], nullptr, 0);
      std::printf("%d %d %llu\n", abc::keyed::ternary(lo), abc::keyed::ternary(hi), (unsigned long long)abc::keyed::uniform_q(lo, hi, q));
    }
    return 0;
  }
  std::fprintf(stderr, "usage: %s small <keyhex> <nonce> <n> <count> | edge <lo> <hi> <q> ...\n", argv[0]);
  return 2;
}
