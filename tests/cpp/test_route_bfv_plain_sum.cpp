// abc_amd/csrc/abc_route.hpp, route_bfv_plain_sum and route_bfv_matvec_bsgs: the BFV plaintext-weighted sum with one inverse
// transform.  plainsum=fused where bfv_multiply_plain takes its fused kernel -- rings 2^10 .. 2^14, every DATA prime below 2^50,
// fp64 on, no ABC_HIP_NO_FUSED, and at N = 2^14 more than 48 ciphertext limbs (count * 2 * L) -- else plainsum=ntt_domain.  Both
// sides of every condition; the arena polynomials and the groups of a call; the matvec's string; format_op as it was.
#include <string>
#include <vector>

#include "../../abc_amd/csrc/abc_route.hpp"
#include "mini_test.hpp"

using namespace abc;
constexpr int BFV = 1, CKKS = 2;

static RouteFacts facts(int scheme, int logn, const std::vector<int> &bits) {
  RouteFacts f;
  f.scheme = scheme; f.logn = logn; f.K = (int)bits.size(); f.L = f.K - 1; f.nB = f.L; f.behz_fp = true;
  for (int j = 0; j < f.K; j++) f.bits[j] = (unsigned char)bits[j];
  f.finish();
  return f;
}
static std::string sum(const RouteFacts &f, size_t count = 1) {
  char b[160];
  if (format_bfv_plain_sum(b, sizeof b, f, count) < 0) throw std::runtime_error("format_bfv_plain_sum failed");
  return b;
}
static std::string bsgs(const RouteFacts &f, size_t count = 1) {
  char b[160];
  if (format_bfv_matvec_bsgs(b, sizeof b, f, count) < 0) throw std::runtime_error("format_bfv_matvec_bsgs failed");
  return b;
}
static std::string op(const RouteFacts &f, int which, int nl, size_t count = 1, bool in_place = false) {
  char b[160];
  if (format_op(b, sizeof b, f, which, nl, count, in_place) < 0) throw std::runtime_error("format_op failed");
  return b;
}
static void eq(const std::string &got, const std::string &want, int line) {
  if (got != want) throw std::runtime_error("line " + std::to_string(line) + ": got \"" + got + "\" want \"" + want + "\"");
}
#define EQ(got, want) eq(got, want, __LINE__)
constexpr BfvPlainSum FUSED = BfvPlainSum::fused, NTTD = BfvPlainSum::ntt_domain;

int main() {
  MiniTest t;
  const std::vector<int> D4096{36, 36, 37}, SMALL{40, 40, 50}, EDGE{49, 49, 50}, WIDE0{60, 40, 60}, D16384{48, 48, 48, 49, 49, 49, 49, 49, 49};

  t.run("the ring: 2^10 .. 2^14 fused, 2^9 and 2^15 .. 2^16 not", [&] {
    for (int logn = 9; logn <= 16; logn++)
      EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, logn, SMALL), 1024) == (logn >= 10 && logn <= 14 ? FUSED : NTTD));
  });

  t.run("prime widths: every DATA prime at most 50 bits; the special prime does not count", [&] {
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, SMALL), 3) == FUSED);
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, EDGE), 3) == FUSED);
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, {50, 50, 50}), 3) == FUSED);
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, {50, 51, 50}), 3) == NTTD);
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, {51, 50, 50}), 3) == NTTD);
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, WIDE0), 3) == NTTD);
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 10, {40, 40, 60}), 3) == FUSED);  // a 60-bit special prime: no data limb
    EXPECT_TRUE(route_bfv_plain_sum(facts(BFV, 12, D4096), 1) == FUSED);
  });

  t.run("switches: ABC_HIP_NO_FUSED and no fp64 take the general route; no other switch matters", [&] {
    RouteFacts f = facts(BFV, 12, D4096);
    f.sw.no_fused = true;
    EXPECT_TRUE(route_bfv_plain_sum(f, 64) == NTTD);
    f = facts(BFV, 12, D4096);
    f.use_fp = false;
    f.finish();
    EXPECT_TRUE(route_bfv_plain_sum(f, 64) == NTTD);
    f = facts(BFV, 12, D4096);
    f.sw.no_split = f.sw.no_bsplit = f.sw.no_plain_mac_sum = f.sw.no_tensor_intt = f.sw.no_mixed = f.sw.no_isplit = f.sw.no_gsplit = true;
    EXPECT_TRUE(route_bfv_plain_sum(f, 64) == FUSED);
  });

  t.run("N = 2^14: bfv_multiply_plain's rule for small launches, count * 2 * L > 48", [&] {
    const RouteFacts f = facts(BFV, 14, D16384);  // L = 8
    EXPECT_TRUE(f.L == 8);
    EXPECT_TRUE(route_bfv_plain_sum(f, 1) == NTTD);
    EXPECT_TRUE(route_bfv_plain_sum(f, 3) == NTTD);   // 48 limbs
    EXPECT_TRUE(route_bfv_plain_sum(f, 4) == FUSED);  // 64
    EXPECT_TRUE(route_bfv_plain_sum(f, 256) == FUSED);
    const RouteFacts g = facts(BFV, 14, SMALL);  // L = 2
    EXPECT_TRUE(route_bfv_plain_sum(g, 12) == NTTD && route_bfv_plain_sum(g, 13) == FUSED);
    const RouteFacts h = facts(BFV, 13, {43, 43, 44, 44, 44});  // the rule is N = 2^14's alone
    EXPECT_TRUE(route_bfv_plain_sum(h, 1) == FUSED);
    EQ(sum(f, 3), "plainsum=ntt_domain");
    EQ(sum(f, 4), "plainsum=fused");
  });

  t.run("arena polynomials per ciphertext", [&] {
    // fused: the partial sum between launches, only where the terms do not fit one launch
    for (bool ntt : {false, true})
      for (bool addend : {false, true}) {
        EXPECT_TRUE(bfv_plain_sum_arena_polys(FUSED, ntt, 1, 2, addend) == 0);
        EXPECT_TRUE(bfv_plain_sum_arena_polys(FUSED, ntt, 8, 3, addend) == 0);
        EXPECT_TRUE(bfv_plain_sum_arena_polys(FUSED, ntt, 9, 2, addend) == 2);
        EXPECT_TRUE(bfv_plain_sum_arena_polys(FUSED, ntt, 25, 3, addend) == 3);
      }
    // ntt_domain: up to eight transformed terms, and the sum under an addend
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, false, 1, 2, false) == 2);
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, false, 5, 2, true) == 12);
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, false, 8, 3, false) == 24);
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, false, 9, 3, false) == 24);
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, false, 25, 2, true) == 18);
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, true, 25, 2, false) == 0);  // NTT-form terms: no forward transform, the sum in d_out
    EXPECT_TRUE(bfv_plain_sum_arena_polys(NTTD, true, 25, 3, true) == 3);
  });

  t.run("groups keep the arenas within 4 GiB", [&] {
    const RouteFacts f = facts(BFV, 15, {55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55, 55});  // L = 15: 3.75 MiB per polynomial
    const size_t poly = (size_t)15 * 32768 * 8;
    for (size_t polys : {(size_t)0, (size_t)2, (size_t)3, (size_t)12, (size_t)18, (size_t)27})
      for (size_t count : {(size_t)0, (size_t)1, (size_t)7, (size_t)64, (size_t)1000, (size_t)100000}) {
        const size_t g = bfv_plain_sum_group(f, count, polys);
        EXPECT_TRUE(g <= count && (g >= 1 || !count));
        EXPECT_TRUE(!polys || g * polys * poly <= ((size_t)4 << 30) || g == 1);
        EXPECT_TRUE(!polys ? g == count : g == count || (g + 1) * polys * poly > ((size_t)4 << 30));  // as large as the cap allows
      }
    EXPECT_TRUE(bfv_plain_sum_group(f, 64, 18) == 60);    // 4 GiB / (18 * 3.75 MiB) = 60.6
    EXPECT_TRUE(bfv_plain_sum_group(f, 64, 16) == 64);    // 3.75 GiB: one group
    EXPECT_TRUE(bfv_plain_sum_group(f, 64, 0) == 64);
    RouteFacts huge = f;
    huge.logn = 16;
    EXPECT_TRUE(bfv_plain_sum_group(huge, 5, 600) == 1);  // one ciphertext passes the cap: still one at a time
  });

  t.run("the matvec: the rotation's route of the ring, plainsum= of the group, add= of rotate_add", [&] {
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : {D4096, SMALL, EDGE, WIDE0, D16384})
        for (size_t count : {(size_t)1, (size_t)3, (size_t)4, (size_t)64}) {
          const RouteFacts f = facts(BFV, logn, bits);
          const size_t group = matvec_bsgs_group(f, f.L, count, 1);
          const BfvMatvecBsgsRoute r = route_bfv_matvec_bsgs(f, group);
          const RotRoute rot = route_rotate(f, f.L, false);
          const RotTailRoute radd = route_rotate_add(f, f.L, false);
          EXPECT_TRUE(r.baby.fold == rot.fold && r.baby.ks.seq == rot.ks.seq && r.baby.ks.front == rot.ks.front);
          EXPECT_TRUE(r.giant.fused == radd.fused && r.sum == route_bfv_plain_sum(f, group));
          EQ(bsgs(f, count), op(f, kRouteRotate, f.L, group) + " plainsum=" + name(r.sum) + " add=" + (radd.fused ? "fused" : "separate"));
        }
    EQ(bsgs(facts(BFV, 12, D4096), 2), "permute lds_fp plainsum=fused add=separate");
    EQ(bsgs(facts(BFV, 14, D16384), 2), "fold bsplit14 pass0=per_target plainsum=ntt_domain add=fused");
    EQ(bsgs(facts(BFV, 14, D16384), 64), "fold bsplit14 pass0=per_limb plainsum=fused add=fused");
    EQ(bsgs(facts(BFV, 13, {43, 43, 44, 44, 44}), 2), "fold bsplit_big plainsum=fused add=fused");
  });

  t.run("numbers 14 and 15, a short buffer; format_op and the CKKS sum as they were", [&] {
    char b[160];
    volatile size_t cap = 8;
    const RouteFacts f = facts(BFV, 14, D16384);
    EXPECT_TRUE(kRouteBfvPlainSum == 14 && kRouteBfvMatvecBsgs == 15);  // include/abc_hip.h: ABC_HIP_ROUTE_BFV_PLAIN_SUM, ..._BFV_MATVEC_BSGS
    EXPECT_TRUE(format_bfv_plain_sum(b, cap, f, 1) == -1 && format_bfv_matvec_bsgs(b, cap, f, 1) == -1);
    RouteFacts longest = f;
    longest.sw.no_rotate_add_fusion = true;
    EXPECT_TRUE(format_bfv_matvec_bsgs(b, 80, longest, 1) > 0);  // the header's promise: 80 bytes hold any route
    for (int unassigned : {6, 8, 9, 11, 13, 14, 15})
      EXPECT_TRUE(format_op(b, sizeof b, f, unassigned, 8, 1, false) == -2);
    EXPECT_TRUE(!route_plain_mac_sum(f, 8) && route_plain_mac_sum(facts(CKKS, 14, SMALL), 2));  // the CKKS call keeps refusing BFV
  });
  return t.summary();
}
