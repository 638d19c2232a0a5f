// abc_amd/csrc/abc_route.hpp, route_matvec_bsgs and route_plain_mac_sum: a matrix-vector product by diagonals, baby-step giant-step.
// The string is the baby rotation's route (format_op(.., kRouteRotate, ..) out of place, for the first group of ciphertexts), then
// " macsum=kernel" -- CKKS on every ring 2^10 .. 2^16, chain and level: one K-term kernel -- or " macsum=per_term"
// (ABC_HIP_NO_PLAIN_MAC_SUM), then the giant step's " add=fused" / " add=separate" (route_rotate_add, out of place).  Also here: the
// groups the batch is walked in (matvec_bsgs_group; mul_sum_group as it was), and that every other route is what it was.
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
  char b[160];
  if (format_op(b, sizeof b, f, which, nl, count, in_place) < 0) throw std::runtime_error("format_op failed");
  return b;
}
static std::string bsgs(const RouteFacts &f, int nl, size_t count = 1) {
  char b[160];
  if (format_matvec_bsgs(b, sizeof b, f, nl, count) < 0) throw std::runtime_error("format_matvec_bsgs failed");
  return b;
}
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
      SW(no_rotate_add_fusion), SW(no_rotate_mac_fusion), SW(no_mulplain_rescale_fusion), SW(no_tensor_sum), Set([](RouteFacts &f) { f.use_fp = false; }),
  };
  const std::vector<std::vector<int>> chains = {FP, MIXED, WIDE, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, {50, 40, 50}, {36, 36, 37}, {50, 50, 50, 50}};

  t.run("macsum=kernel for CKKS on every ring, chain, level and switch; the rotations are the level's", [&] {
    size_t n = 0;
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches)
          for (int nl = 1; nl <= (int)bits.size() - 1; nl++) {
            RouteFacts f = facts(CKKS, logn, bits);
            set(f);
            f.finish();
            const MatvecBsgsRoute r = route_matvec_bsgs(f, nl);
            const RotRoute rot = route_rotate(f, nl, false);
            const RotTailRoute radd = route_rotate_add(f, nl, false);
            EXPECT_TRUE(r.macsum && route_plain_mac_sum(f, nl));
            EXPECT_TRUE(r.baby.fold == rot.fold && r.baby.ks.seq == rot.ks.seq && r.baby.ks.front == rot.ks.front);
            EXPECT_TRUE(r.giant.fused == radd.fused && r.giant.rot.fold == radd.rot.fold && r.giant.rot.ks.seq == radd.rot.ks.seq);
            for (size_t count : {(size_t)1, (size_t)3, (size_t)32, (size_t)256})  // one group: the rotation's string for the whole call
              EQ(bsgs(f, nl, count), op(f, kRouteRotate, nl, count) + " macsum=kernel add=" + (radd.fused ? "fused" : "separate"));
            f.sw.no_plain_mac_sum = true;
            EXPECT_TRUE(!route_matvec_bsgs(f, nl).macsum && !route_plain_mac_sum(f, nl));
            EQ(bsgs(f, nl, 32), op(f, kRouteRotate, nl, 32) + " macsum=per_term add=" + (radd.fused ? "fused" : "separate"));
            n++;
          }
    EXPECT_TRUE(n > 2000);
  });

  t.run("the documented strings", [&] {
    EQ(bsgs(facts(CKKS, 14, FP), 4, 2), "fold split14 front=lean pack=1 main=split4 macsum=kernel add=fused");
    EQ(bsgs(facts(CKKS, 14, FP), 3, 512), "fold split14 front=fat pack=1 main=split4 macsum=kernel add=fused");
    EQ(bsgs(facts(CKKS, 14, MIXED), 3), "fold isplit14 guard=1 fpmask=0x6 macsum=kernel add=separate");
    EQ(bsgs(facts(CKKS, 15, FP), 3), "fold gsplit15 macsum=kernel add=fused");
    EQ(bsgs(facts(CKKS, 15, {50, 40, 40, 40, 40, 40, 40, 40, 40, 50}), 8), "fold gsplit15 macsum=kernel add=separate");  // the deep main kernel takes no addend
    EQ(bsgs(facts(CKKS, 12, FP), 4), "permute lds_fp macsum=kernel add=separate");
    EQ(bsgs(facts(CKKS, 10, FP), 4), "permute lds_fp macsum=kernel add=separate");
    EQ(bsgs(facts(CKKS, 16, FP), 4), "permute generic front=fp macsum=kernel add=separate");
    RouteFacts g = facts(CKKS, 14, FP);
    g.sw.no_split = true;
    EQ(bsgs(g, 4), "permute lds_fp macsum=kernel add=separate");
    g = facts(CKKS, 14, FP);
    g.sw.no_rotate_add_fusion = true;
    EQ(bsgs(g, 4), "fold split14 front=lean pack=1 main=split4 macsum=kernel add=separate");
    g = facts(CKKS, 14, FP);
    g.sw.no_galois_fusion = true;
    EQ(bsgs(g, 4), "permute split14 front=lean pack=1 main=split4 macsum=kernel add=separate");
    g = facts(CKKS, 14, FP);
    g.sw.no_plain_mac_sum = true;
    EQ(bsgs(g, 4, 2), "fold split14 front=lean pack=1 main=split4 macsum=per_term add=fused");
  });

  t.run("groups: the rule of mul_sum_relin with 2 * n_baby polynomials per ciphertext; mul_sum_group as it was", [&] {
    const RouteFacts f = facts(CKKS, 14, FP);
    for (int nb : {0, 1, 4, 8, 64})
      for (size_t count : {(size_t)1, (size_t)5, (size_t)8, (size_t)9, (size_t)100, (size_t)512, (size_t)8192, (size_t)100000}) {
        const ChunkPlan p = plan_chunks(f, 3, count);
        const size_t g = matvec_bsgs_group(f, 3, count, nb), unit = p.chunk * (size_t)p.lanes, polys = 2 * (size_t)(nb ? nb : 1);
        EXPECT_TRUE(g >= 1 && g <= count);
        EXPECT_TRUE(g == count || g % unit == 0);
        EXPECT_TRUE(g * polys * 3 * 16384 * 8 <= ((size_t)4 << 30) || g == unit);
      }
    EXPECT_TRUE(matvec_bsgs_group(f, 3, 512, 4) == 512);  // 1.5 GiB of rotated ciphertexts: one group
    EXPECT_TRUE(matvec_bsgs_group(f, 3, 512, 8) == 512);  // 3 GiB
    EXPECT_TRUE(matvec_bsgs_group(f, 3, 512, 16) == 256);  // 6 GiB would pass the cap: 4 GiB / 12 MiB = 341 ciphertexts, in units of 128 * 2
    EXPECT_TRUE(mul_sum_group(f, 4, 512) == 512);
    EXPECT_TRUE(mul_sum_group(f, 4, 8192) == 2560);
    RouteFacts c2 = f;
    c2.sw.chunk = 2;
    EXPECT_TRUE(matvec_bsgs_group(c2, 3, 5, 4) == 2);  // up to eight ciphertexts run on one lane
    EXPECT_TRUE(matvec_bsgs_group(c2, 3, 11, 4) == 4);  // two lanes
    c2.sw.lanes = 1;
    EXPECT_TRUE(matvec_bsgs_group(c2, 3, 11, 4) == 2);
    EXPECT_TRUE(matvec_bsgs_group(c2, 3, 1, 4) == 1);
    c2.sw.lanes = 2;
    EQ(bsgs(c2, 3, 5), op(c2, kRouteRotate, 3, 2) + " macsum=kernel add=fused");  // the string of a call in several groups is the first group's
  });

  t.run("every other route gives the string it gave, under the new switch too", [&] {
    for (int scheme : {BFV, CKKS})
      for (int logn = 10; logn <= 16; logn++)
        for (const std::vector<int> &bits : chains)
          for (int nl = (scheme == BFV ? (int)bits.size() - 1 : 1); nl <= (int)bits.size() - 1; nl++)
            for (int which : {(int)kRouteMulRelin, (int)kRouteKeyswitch, (int)kRouteRotate, (int)kRouteRescale, (int)kRouteMultiply, (int)kRouteRotateAdd,
                              (int)kRouteRotateMacPlain, (int)kRouteMulPlainRescale, (int)kRouteMulSumRelin})
              for (bool in_place : {false, true}) {
                if ((which == kRouteRescale || which == kRouteMulPlainRescale) && (scheme == BFV || nl < 2)) continue;
                RouteFacts f = facts(scheme, logn, bits), g = f;
                g.sw.no_plain_mac_sum = true;
                EQ(op(g, which, nl, 64, in_place), op(f, which, nl, 64, in_place));
              }
    EQ(op(facts(CKKS, 14, FP), kRouteMulSumRelin, 4, 2), "split14 front=lean pack=1 main=split4 tensor=sum");
    EXPECT_TRUE(!route_plain_mac_sum(facts(BFV, 12, {36, 36, 37}), 2));  // no BFV plaintext sum: the C ABI refuses the call
  });

  t.run("op 13 has its own formatter, a short buffer; format_op knows the operations it knew", [&] {
    char b[160];
    volatile size_t cap = 8;
    const RouteFacts f = facts(CKKS, 14, FP);
    EXPECT_TRUE(kRouteDiagMatvecBsgs == 13);  // include/abc_hip.h: ABC_HIP_ROUTE_DIAG_MATVEC_BSGS
    EXPECT_TRUE(format_matvec_bsgs(b, sizeof b, f, 4, 1) > 0);
    RouteFacts longest = f;
    longest.sw.no_plain_mac_sum = longest.sw.no_rotate_add_fusion = true;
    EXPECT_TRUE(format_matvec_bsgs(b, 80, longest, 4, 1) > 0);  // the header's promise: 80 bytes hold any route
    EXPECT_TRUE(format_matvec_bsgs(b, cap, f, 4, 1) == -1);
    for (int unassigned : {6, 8, 9, 11, 13, 14})  // 13 is abc_hip_route's to dispatch, not format_op's
      EXPECT_TRUE(format_op(b, sizeof b, f, unassigned, 4, 1, false) == -2);
  });
  return t.summary();
}
