// abc_amd/csrc/abc_route.hpp, route_plain_sum_rescale and route_matvec_bsgs_rescale: where rescale(addend + sum of plaintext products)
// forms the sum in the rescale's own loads.  Over every ring 2^10 .. 2^16, chains whose primes are all fp64-capable, mixed and 60-bit
// ones, every level and every switch, `fused` is true exactly where route_rescale (out of place) gives the LDS-resident kernels -- fp
// or mixed -- and neither ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION nor ABC_HIP_NO_PLAIN_MAC_SUM is set, for a short sum on a large batch;
// the measured rule beyond that (profiles/plain_sum_rescale_ab.log: up to four terms, a workgroup per CU and 2^20 coefficients in
// R1), and ABC_HIP_PLAIN_SUM_RESCALE_TERMS, which takes the measurement out; string 16 is the rescale's plus " sumrescale=fused" /
// " sumrescale=separate"; string 17 is the baby rotation's route at nl, sumrescale=, and the giant step's route at nl - 1 with add=;
// how many terms the streaming kernel takes first; and every other route is what it was.
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
static std::string psr(const RouteFacts &f, int nl, size_t count = 1024) {
  char b[80];
  if (format_plain_sum_rescale(b, sizeof b, f, nl, count) < 0) throw std::runtime_error("format_plain_sum_rescale failed");
  return b;
}
static std::string bsgs(const RouteFacts &f, int nl, size_t count = 1) {
  char b[160];
  if (format_matvec_bsgs_rescale(b, sizeof b, f, nl, count) < 0) throw std::runtime_error("format_matvec_bsgs_rescale failed");
  return b;
}
static RouteFacts forced(RouteFacts f, int terms = 8) {  // ABC_HIP_PLAIN_SUM_RESCALE_TERMS
  f.sw.plain_sum_rescale_terms = terms;
  return f;
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
      SW(no_rotate_add_fusion), SW(no_rotate_mac_fusion), SW(no_mulplain_rescale_fusion), SW(no_tensor_sum), SW(no_plain_mac_sum),
      SW(no_plain_sum_rescale_fusion), Set([](RouteFacts &f) { f.use_fp = false; }),
      Set([](RouteFacts &f) { f.sw.no_plain_sum_rescale_fusion = f.sw.no_fused = true; }),
      Set([](RouteFacts &f) { f.sw.no_plain_sum_rescale_fusion = f.sw.no_plain_mac_sum = true; }),
      Set([](RouteFacts &f) { f.sw.no_plain_mac_sum = f.sw.no_mixed = true; }),
  };
  const std::vector<std::vector<int>> chains = {FP, MIXED, WIDE, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, {50, 40, 50}, {36, 36, 37}, {50, 50, 50, 50}};

  t.run("fused exactly on the LDS-resident rescale without either switch, and both strings say so", [&] {
    size_t fused_n = 0, separate_n = 0;
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches)
          for (int nl = 2; nl <= (int)bits.size() - 1; nl++) {
            RouteFacts f = facts(CKKS, logn, bits);
            set(f);
            f.finish();
            const PlainSumRescaleRoute r = route_plain_sum_rescale(f, nl);  // a short sum on a large batch
            const RescaleRoute rs = route_rescale(f, nl, false);
            EXPECT_TRUE(r.rescale.kind == rs.kind && r.rescale.fpmask == rs.fpmask);
            // the rule, spelt out: a ring that fits LDS, not ABC_HIP_NO_FUSED, and with a prime above 2^50 (or fp64 off) not
            // ABC_HIP_NO_ISPLIT; then the two switches
            const bool lds = logn >= 10 && logn <= 14 && !f.sw.no_fused && ((f.use_fp && f.data_fp(nl)) || !f.sw.no_isplit);
            EXPECT_TRUE((rs.kind != Rescale::generic) == lds);
            const bool want = lds && !f.sw.no_plain_sum_rescale_fusion && !f.sw.no_plain_mac_sum;
            EXPECT_TRUE(r.fused == want);
            (want ? fused_n : separate_n)++;
            const std::string tail = want ? " sumrescale=fused" : " sumrescale=separate";
            EQ(psr(f, nl), op(f, kRouteRescale, nl) + tail);
            const MatvecBsgsRescaleRoute m = route_matvec_bsgs_rescale(f, nl);
            EXPECT_TRUE(m.sum.fused == want);
            // the switch takes the measurement out: every batch, every number of terms
            for (size_t polys : {(size_t)1, (size_t)6, (size_t)4096})
              for (int k : {1, 4, 5, 25}) EXPECT_TRUE(route_plain_sum_rescale(forced(f), nl, polys, k).fused == want);
            EXPECT_TRUE(!want || (route_plain_sum_rescale(forced(f, 2), nl, 6, 9).fused_terms == 2 && route_plain_sum_rescale(forced(f, 99), nl).fused_terms == 8));
            for (size_t count : {(size_t)1, (size_t)64}) {
              const RouteFacts u = f;
              const RouteFacts f = forced(u);
              const size_t group = matvec_bsgs_group(f, nl, count, 1);
              // the baby rotation as ABC_HIP_ROUTE_ROTATE at nl, the giant step as ABC_HIP_ROUTE_ROTATE_ADD's separate form at nl - 1
              const RotTailRoute g = route_rotate_add(f, nl - 1, false);
              char ks[80];
              format_ks(ks, sizeof ks, f, g.rot.ks, nl - 1, group);
              EQ(bsgs(f, nl, count), op(f, kRouteRotate, nl, group) + tail + (g.rot.fold ? " fold " : " permute ") + ks + (g.fused ? " add=fused" : " add=separate"));
            }
          }
    EXPECT_TRUE(fused_n > 500 && separate_n > 500);
  });

  t.run("the documented strings", [&] {
    for (int logn = 10; logn <= 14; logn++) {
      EQ(psr(facts(CKKS, logn, FP), 4), "fp sumrescale=fused");
      EQ(psr(facts(CKKS, logn, FP), 2), "fp sumrescale=fused");
      EQ(psr(facts(CKKS, logn, MIXED), 3), "mixed fpmask=0x6 sumrescale=fused");
      EQ(psr(facts(CKKS, logn, MIXED), 2), "mixed fpmask=0x2 sumrescale=fused");
      EQ(psr(facts(CKKS, logn, WIDE), 3), "mixed fpmask=0x0 sumrescale=fused");
    }
    for (int logn : {15, 16})
      for (const std::vector<int> &bits : {FP, MIXED, WIDE}) EQ(psr(facts(CKKS, logn, bits), 3), "generic sumrescale=separate");
    RouteFacts g = facts(CKKS, 12, FP);
    g.sw.no_fused = true;
    EQ(psr(g, 4), "generic sumrescale=separate");
    g = facts(CKKS, 12, FP);
    g.sw.no_plain_sum_rescale_fusion = true;
    EQ(psr(g, 4), "fp sumrescale=separate");
    g = facts(CKKS, 12, FP);
    g.sw.no_plain_mac_sum = true;
    EQ(psr(g, 4), "fp sumrescale=separate");
    g = facts(CKKS, 12, MIXED);
    g.sw.no_mixed = true;
    EQ(psr(g, 3), "mixed fpmask=0x0 sumrescale=fused");
    g = facts(CKKS, 14, MIXED);
    g.sw.no_isplit = true;
    EQ(psr(g, 3), "generic sumrescale=separate");
    g = facts(CKKS, 14, FP);
    g.use_fp = false;
    g.finish();
    EQ(psr(g, 4), "mixed fpmask=0x0 sumrescale=fused");

    // the matvec: small batches under ABC_HIP_PLAIN_SUM_RESCALE_TERMS=8, as the parity tests run them, then the rule's own answers
    const std::string split14 = "split14 front=lean pack=1 main=split4", fat14 = "split14 front=fat pack=1 main=split4";
    EQ(bsgs(forced(facts(CKKS, 10, {50, 40, 40, 50})), 3), "permute lds_fp sumrescale=fused permute lds_fp add=separate");
    EQ(bsgs(forced(facts(CKKS, 12, {50, 40, 40, 50})), 3), "permute lds_fp sumrescale=fused permute lds_fp add=separate");
    EQ(bsgs(forced(facts(CKKS, 14, FP)), 3, 2), "fold " + split14 + " sumrescale=fused fold " + split14 + " add=fused");
    EQ(bsgs(forced(facts(CKKS, 14, FP)), 2, 2), "fold " + split14 + " sumrescale=fused fold " + split14 + " add=fused");
    EQ(bsgs(forced(facts(CKKS, 14, MIXED)), 3, 2), "fold isplit14 guard=1 fpmask=0x6 sumrescale=fused fold isplit14 guard=1 fpmask=0x2 add=separate");
    EQ(bsgs(forced(facts(CKKS, 15, {50, 40, 40, 50})), 3, 2), "fold gsplit15 sumrescale=separate fold gsplit15 add=fused");
    g = forced(facts(CKKS, 14, FP));
    g.sw.no_rotate_add_fusion = true;
    EQ(bsgs(g, 3, 2), "fold " + split14 + " sumrescale=fused fold " + split14 + " add=separate");
    g = forced(facts(CKKS, 14, FP));
    g.sw.no_plain_mac_sum = true;
    EQ(bsgs(g, 3, 2), "fold " + split14 + " sumrescale=separate fold " + split14 + " add=fused");
    EQ(bsgs(facts(CKKS, 14, FP), 3, 2), "fold " + split14 + " sumrescale=separate fold " + split14 + " add=fused");
    EQ(bsgs(facts(CKKS, 14, FP), 3, 512), "fold " + fat14 + " sumrescale=fused fold " + fat14 + " add=fused");
  });

  t.run("the measured rule: up to four terms, a workgroup per CU and 2^20 coefficients in R1", [&] {
    EXPECT_TRUE(kPlainSumRescaleTerms == 4 && kPlainSumRescaleMinPolys == 256 && kPlainSumRescaleMinCoeffs == ((size_t)1 << 20));
    const RouteFacts f14 = facts(CKKS, 14, FP), f12 = facts(CKKS, 12, {50, 40, 40, 50}), f10 = facts(CKKS, 10, {50, 40, 40, 50});
    for (int k = 1; k <= 4; k++) {
      EXPECT_TRUE(route_plain_sum_rescale(f14, 4, 256, k).fused && !route_plain_sum_rescale(f14, 4, 255, k).fused);  // batch 128 against 64 measured
      EXPECT_TRUE(route_plain_sum_rescale(f12, 3, 256, k).fused && !route_plain_sum_rescale(f12, 3, 255, k).fused);
      EXPECT_TRUE(route_plain_sum_rescale(f10, 3, 1024, k).fused && !route_plain_sum_rescale(f10, 3, 1023, k).fused);  // 2^20 coefficients
      EXPECT_TRUE(route_plain_sum_rescale(f14, 4, 256, k).fused_terms == 4);
    }
    for (int k : {5, 6, 8, 9, 16, 25}) EXPECT_TRUE(!route_plain_sum_rescale(f14, 4, 1024, k).fused && !route_plain_sum_rescale(f12, 3, 2048, k).fused);
    EQ(psr(f14, 4, 128), "fp sumrescale=fused");  // 256 polynomials of size-2 ciphertexts
    EQ(psr(f14, 4, 127), "fp sumrescale=separate");
    EQ(psr(f14, 4, 3), "fp sumrescale=separate");
    EQ(psr(forced(f14), 4, 3), "fp sumrescale=fused");
    EQ(psr(forced(f14, 0), 4, 3), "fp sumrescale=fused");
    EQ(psr(facts(CKKS, 14, MIXED), 3, 3), "mixed fpmask=0x6 sumrescale=separate");
  });

  t.run("terms the streaming kernel sums first", [&] {
    EXPECT_TRUE(kPlainSumRescaleTerms >= 1 && kPlainSumRescaleTerms <= 8);
    for (int k = 0; k <= kPlainSumRescaleTerms; k++) EXPECT_TRUE(plain_sum_rescale_lead(k, kPlainSumRescaleTerms) == 0);  // the rule's own sums: no leading launch
    for (int k = 0; k <= 8; k++) EXPECT_TRUE(plain_sum_rescale_lead(k, 8) == 0);
    EXPECT_TRUE(plain_sum_rescale_lead(9, 8) == 8 && plain_sum_rescale_lead(16, 8) == 8 && plain_sum_rescale_lead(17, 8) == 16);
    EXPECT_TRUE(plain_sum_rescale_lead(24, 8) == 16 && plain_sum_rescale_lead(25, 8) == 24);
    // a lower number of fused terms: whole launches first, the fused pair never gets more than it takes, and a carry alone is allowed
    EXPECT_TRUE(plain_sum_rescale_lead(4, 4) == 0 && plain_sum_rescale_lead(5, 4) == 5 && plain_sum_rescale_lead(12, 4) == 8);
    EXPECT_TRUE(plain_sum_rescale_lead(1, 1) == 0 && plain_sum_rescale_lead(2, 1) == 2 && plain_sum_rescale_lead(9, 1) == 8);
    for (int fused = 1; fused <= 8; fused++)
      for (int k = 0; k <= 40; k++) {
        const int lead = plain_sum_rescale_lead(k, fused);
        EXPECT_TRUE(lead >= 0 && lead <= k && k - lead <= fused && (lead % 8 == 0 || lead == k));
      }
  });

  t.run("every other route gives the string it gave, under the new switch too", [&] {
    for (int scheme : {BFV, CKKS})
      for (int logn = 10; logn <= 16; logn++)
        for (const std::vector<int> &bits : chains)
          for (int nl = (scheme == BFV ? (int)bits.size() - 1 : 1); nl <= (int)bits.size() - 1; nl++)
            for (bool in_place : {false, true}) {
              RouteFacts f = facts(scheme, logn, bits), g = f;
              g.sw.no_plain_sum_rescale_fusion = true;
              for (int which : {(int)kRouteMulRelin, (int)kRouteKeyswitch, (int)kRouteRotate, (int)kRouteRescale, (int)kRouteMultiply, (int)kRouteRotateAdd,
                                (int)kRouteRotateMacPlain, (int)kRouteMulPlainRescale, (int)kRouteMulSumRelin}) {
                if ((which == kRouteRescale || which == kRouteMulPlainRescale) && (scheme == BFV || nl < 2)) continue;
                EQ(op(g, which, nl, 64, in_place), op(f, which, nl, 64, in_place));
              }
              if (scheme == CKKS) {
                char a[160], b[160];
                EXPECT_TRUE(format_matvec_bsgs(a, sizeof a, f, nl, 64) > 0 && format_matvec_bsgs(b, sizeof b, g, nl, 64) > 0 && std::string(a) == b);
              }
            }
    EQ(op(facts(CKKS, 14, FP), kRouteMulPlainRescale, 4), "fp mulplain=fused");
  });

  t.run("the op numbers, short buffers; format_op knows the operations it knew", [&] {
    char b[200];
    volatile size_t cap = 8;
    const RouteFacts f = facts(CKKS, 14, FP);
    EXPECT_TRUE(kRoutePlainSumRescale == 16 && kRouteDiagMatvecBsgsRescale == 17);  // include/abc_hip.h: ABC_HIP_ROUTE_PLAIN_SUM_RESCALE, ..._DIAG_MATVEC_BSGS_RESCALE
    EXPECT_TRUE(format_plain_sum_rescale(b, cap, f, 4, 1) == -1 && format_matvec_bsgs_rescale(b, cap, f, 4, 1) == -1);
    RouteFacts longest = facts(CKKS, 14, WIDE);
    longest.sw.no_plain_mac_sum = longest.sw.no_rotate_add_fusion = true;
    EXPECT_TRUE(format_plain_sum_rescale(b, 80, longest, 3, 1) > 0);
    EXPECT_TRUE(format_matvec_bsgs_rescale(b, 160, longest, 3, 1) > 0);  // the header's promise: 160 bytes hold any route of 17
    longest = f;
    longest.sw.no_plain_mac_sum = longest.sw.no_rotate_add_fusion = true;
    EXPECT_TRUE(format_matvec_bsgs_rescale(b, 160, longest, 4, 1) > 0);
    for (int unassigned : {6, 8, 9, 11, 13, 14, 15, 16, 17})  // 13 .. 17 are abc_hip_route's to dispatch, not format_op's
      EXPECT_TRUE(format_op(b, sizeof b, f, unassigned, 4, 1, false) == -2);
  });
  return t.summary();
}
