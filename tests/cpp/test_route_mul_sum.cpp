// abc_amd/csrc/abc_route.hpp, route_mul_sum: relinearize(sum of ciphertext products).  The key switch is the one of the level
// (route_keyswitch; its string is format_op(.., kRouteKeyswitch, ..) for the first group of ciphertexts), followed by " tensor=sum"
// -- CKKS on every ring 2^10 .. 2^16 and every chain, one K-term kernel -- or " tensor=per_term": BFV, whose product rounds, and
// ABC_HIP_NO_TENSOR_SUM.  Also here: the groups the batch is walked in (mul_sum_group), and that every other route is what it was.
#include <functional>
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
static std::string op(const RouteFacts &f, int which, int nl, size_t count = 1, bool in_place = false) {
  char b[128];
  if (format_op(b, sizeof b, f, which, nl, count, in_place) < 0) throw std::runtime_error("format_op failed");
  return b;
}
static std::string msr(const RouteFacts &f, int nl, size_t count = 1) { return op(f, kRouteMulSumRelin, nl, count); }
static void eq(const std::string &got, const std::string &want, int line) {
  if (got != want) throw std::runtime_error("line " + std::to_string(line) + ": got \"" + got + "\" want \"" + want + "\"");
}
#define EQ(got, want) eq(got, want, __LINE__)

using Set = std::function<void(RouteFacts &)>;
#define SW(field) Set([](RouteFacts &f) { f.sw.field = true; })

int main() {
  MiniTest t;
  const std::vector<int> FP{50, 40, 40, 40, 50}, MIXED{60, 40, 40, 60}, WIDE{60, 60, 60, 60};
  const std::vector<Set> switches = {
      Set([](RouteFacts &) {}), SW(no_fused), SW(no_split), SW(no_split4), SW(no_isplit), SW(no_gsplit), SW(no_lean_front), SW(no_bsplit),
      SW(no_mixed), SW(no_pack), SW(no_key_twin), SW(no_bmul), SW(no_iks), SW(no_tensor_intt), SW(no_galois_fusion), SW(main_two_per_cu),
      SW(no_rotate_add_fusion), SW(no_rotate_mac_fusion), SW(no_mulplain_rescale_fusion), Set([](RouteFacts &f) { f.use_fp = false; }),
  };
  const std::vector<std::vector<int>> chains = {FP, MIXED, WIDE, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, {50, 40, 50}, {36, 36, 37}, {50, 50, 50, 50}};

  t.run("tensor=sum for CKKS on every ring, chain and switch; the key switch is the level's", [&] {
    size_t n = 0;
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches)
          for (int nl = 1; nl <= (int)bits.size() - 1; nl++) {
            RouteFacts f = facts(CKKS, logn, bits);
            set(f);
            f.finish();
            const MulSumRoute r = route_mul_sum(f, nl);
            const KsRoute ks = route_keyswitch(f, nl);
            EXPECT_TRUE(r.sum);
            EXPECT_TRUE(r.ks.seq == ks.seq && r.ks.front == ks.front);
            for (size_t count : {(size_t)1, (size_t)3, (size_t)32, (size_t)256})  // one group: the key switch's string for the whole call
              EQ(msr(f, nl, count), op(f, kRouteKeyswitch, nl, count) + " tensor=sum");
            f.sw.no_tensor_sum = true;
            EXPECT_TRUE(!route_mul_sum(f, nl).sum);
            EQ(msr(f, nl, 32), op(f, kRouteKeyswitch, nl, 32) + " tensor=per_term");
            n++;
          }
    EXPECT_TRUE(n > 2000);
  });

  t.run("tensor=per_term for BFV", [&] {
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches) {
          RouteFacts f = facts(BFV, logn, bits);
          set(f);
          f.finish();
          const int nl = f.L;
          EXPECT_TRUE(!route_mul_sum(f, nl).sum);
          EQ(msr(f, nl, 4), op(f, kRouteKeyswitch, nl, 4) + " tensor=per_term");
        }
  });

  t.run("the documented strings", [&] {
    EQ(msr(facts(CKKS, 14, FP), 4, 2), "split14 front=lean pack=1 main=split4 tensor=sum");
    EQ(msr(facts(CKKS, 14, FP), 4, 512), "split14 front=fat pack=1 main=split4 tensor=sum");
    EQ(msr(facts(CKKS, 14, MIXED), 3), "isplit14 guard=1 fpmask=0x6 tensor=sum");
    EQ(msr(facts(CKKS, 15, FP), 3), "gsplit15 tensor=sum");
    EQ(msr(facts(CKKS, 12, FP), 4), "lds_fp tensor=sum");
    EQ(msr(facts(CKKS, 10, FP), 4), "lds_fp tensor=sum");
    EQ(msr(facts(CKKS, 16, FP), 4), "generic front=fp tensor=sum");
    RouteFacts g = facts(CKKS, 14, FP);
    g.sw.no_split = true;
    EQ(msr(g, 4), "lds_fp tensor=sum");
    g = facts(CKKS, 14, FP);
    g.sw.no_fused = true;
    EQ(msr(g, 4), "generic front=plain tensor=sum");
    g = facts(CKKS, 14, FP);
    g.sw.no_tensor_sum = true;
    EQ(msr(g, 4, 2), "split14 front=lean pack=1 main=split4 tensor=per_term");
    EQ(msr(facts(BFV, 14, {50, 50, 50, 50, 50, 50, 50, 50, 50}), 8), op(facts(BFV, 14, {50, 50, 50, 50, 50, 50, 50, 50, 50}), kRouteKeyswitch, 8) + " tensor=per_term");
  });

  t.run("groups: a multiple of chunk * lanes, the arena within 4 GiB, ABC_HIP_CHUNK exactly", [&] {
    const RouteFacts f = facts(CKKS, 14, FP);
    for (size_t count : {(size_t)1, (size_t)5, (size_t)8, (size_t)9, (size_t)100, (size_t)512, (size_t)8192, (size_t)100000}) {
      const ChunkPlan p = plan_chunks(f, 4, count);
      const size_t g = mul_sum_group(f, 4, count), unit = p.chunk * (size_t)p.lanes;
      EXPECT_TRUE(g >= 1 && g <= count);
      EXPECT_TRUE(g == count || g % unit == 0);
      EXPECT_TRUE(g * 3 * 4 * 16384 * 8 <= ((size_t)4 << 30) || g == unit);
    }
    EXPECT_TRUE(mul_sum_group(f, 4, 512) == 512);    // one group: the key switch chunks as it does in relinearize
    EXPECT_TRUE(mul_sum_group(f, 4, 8192) == 2560);  // 4 GiB / 1.5 MiB = 2730 ciphertexts, in units of 128 * 2
    RouteFacts c2 = f;
    c2.sw.chunk = 2;
    EXPECT_TRUE(mul_sum_group(c2, 4, 5) == 2);  // up to eight ciphertexts run on one lane
    EXPECT_TRUE(mul_sum_group(c2, 4, 7) == 2);
    EXPECT_TRUE(mul_sum_group(c2, 4, 9) == 4);  // two lanes
    c2.sw.lanes = 1;
    EXPECT_TRUE(mul_sum_group(c2, 4, 9) == 2);
    EXPECT_TRUE(mul_sum_group(c2, 4, 1) == 1);
    // the string of a call in several groups is the first group's: five ciphertexts in chunks of two
    EQ(msr(c2, 4, 5), op(c2, kRouteKeyswitch, 4, 2) + " tensor=sum");
  });

  t.run("every other route gives the string it gave, under the new switch too", [&] {
    for (int scheme : {BFV, CKKS})
      for (int logn = 10; logn <= 16; logn++)
        for (const std::vector<int> &bits : chains)
          for (int nl = (scheme == BFV ? (int)bits.size() - 1 : 1); nl <= (int)bits.size() - 1; nl++)
            for (int which : {(int)kRouteMulRelin, (int)kRouteKeyswitch, (int)kRouteRotate, (int)kRouteRescale, (int)kRouteMultiply, (int)kRouteRotateAdd,
                              (int)kRouteRotateMacPlain, (int)kRouteMulPlainRescale})
              for (bool in_place : {false, true}) {
                if ((which == kRouteRescale || which == kRouteMulPlainRescale) && (scheme == BFV || nl < 2)) continue;
                RouteFacts f = facts(scheme, logn, bits), g = f;
                g.sw.no_tensor_sum = true;
                EQ(op(g, which, nl, 64, in_place), op(f, which, nl, 64, in_place));
              }
    EQ(op(facts(CKKS, 14, FP), kRouteMulRelin, 4), "split14 front=lean pack=1 main=split4");
  });

  t.run("op 12 is known, a short buffer, the unassigned numbers", [&] {
    char b[96];
    volatile size_t cap = 8;
    const RouteFacts f = facts(CKKS, 14, FP);
    EXPECT_TRUE(kRouteMulSumRelin == 12);  // include/abc_hip.h: ABC_HIP_ROUTE_MUL_SUM_RELIN
    EXPECT_TRUE(format_op(b, sizeof b, f, 12, 4, 1, false) > 0);
    EXPECT_TRUE(format_op(b, cap, f, kRouteMulSumRelin, 4, 1, false) == -1);
    for (int unassigned : {6, 8, 9, 11, 13})
      EXPECT_TRUE(format_op(b, sizeof b, f, unassigned, 4, 1, false) == -2);
  });
  return t.summary();
}
