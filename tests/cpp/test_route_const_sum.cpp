// abc_amd/csrc/abc_route.hpp, the routes of the scalar-weighted sum and of polynomial evaluation: route_const_mac_sum is the K-term
// kernel on every CKKS context unless ABC_HIP_NO_CONST_MAC_SUM says otherwise; route_const_sum_rescale fuses exactly where the rescale
// is LDS-resident, the sum has 1 .. 4 terms that all sit at nl and ABC_HIP_NO_CONST_MAC_SUM is not set -- by the measured rule (64
// polynomials, 2^20 coefficients), or as ABC_HIP_CONST_SUM_RESCALE_FUSED forces it within that; nothing sends a call with a term
// above nl, five terms, N >= 2^15, ABC_HIP_NO_FUSED or ABC_HIP_NO_ISPLIT on a wide chain to the fused pair; string 18 is the rescale's
// route plus constsum=, string 19 the mul_relin route plus constsum=separate; the new switches change no route that existed.
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
static std::string csr(const RouteFacts &f, int nl, size_t count = 1024) {
  char b[80];
  if (format_const_sum_rescale(b, sizeof b, f, nl, count) < 0) throw std::runtime_error("format_const_sum_rescale failed");
  return b;
}
static std::string pe(const RouteFacts &f, int nl, size_t count = 1) {
  char b[160];
  if (format_poly_eval(b, sizeof b, f, nl, count) < 0) throw std::runtime_error("format_poly_eval failed");
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
      SW(no_rotate_add_fusion), SW(no_rotate_mac_fusion), SW(no_mulplain_rescale_fusion), SW(no_tensor_sum), SW(no_plain_mac_sum),
      SW(no_plain_sum_rescale_fusion), SW(no_const_mac_sum), Set([](RouteFacts &f) { f.use_fp = false; }),
      Set([](RouteFacts &f) { f.sw.no_const_mac_sum = f.sw.no_fused = true; }),
      Set([](RouteFacts &f) { f.sw.plain_sum_rescale_terms = 8; }),
  };
  const std::vector<std::vector<int>> chains = {FP, MIXED, WIDE, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, {50, 40, 50}, {36, 36, 37},
                                                {50, 30, 30, 30, 30, 30, 30, 50}};

  t.run("the K-term kernel on CKKS unless the switch says otherwise", [&] {
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (int nl = 1; nl <= (int)bits.size() - 1; nl++) {
          RouteFacts f = facts(CKKS, logn, bits);
          EXPECT_TRUE(route_const_mac_sum(f, nl));
          f.sw.no_plain_mac_sum = f.sw.no_plain_sum_rescale_fusion = f.sw.no_fused = f.sw.no_mixed = true;  // not its switches
          EXPECT_TRUE(route_const_mac_sum(f, nl));
          f.sw.no_const_mac_sum = true;
          EXPECT_TRUE(!route_const_mac_sum(f, nl));
        }
    EXPECT_TRUE(!route_const_mac_sum(facts(BFV, 12, {36, 36, 37}), 2));
  });

  t.run("fused exactly where the pair can run, by the rule or as forced; string 18 says so", [&] {
    size_t fused_n = 0, separate_n = 0;
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches)
          for (int nl = 2; nl <= (int)bits.size() - 1; nl++) {
            RouteFacts f = facts(CKKS, logn, bits);
            set(f);
            f.finish();
            const RescaleRoute rs = route_rescale(f, nl, false);
            const bool can = rs.kind != Rescale::generic && !f.sw.no_const_mac_sum;
            // the rule, spelt out: a ring that fits LDS, not ABC_HIP_NO_FUSED, and with a prime above 2^50 (or fp64 off) not ABC_HIP_NO_ISPLIT
            if (logn > 14 || f.sw.no_fused) EXPECT_TRUE(!can);
            const size_t big = (size_t)1 << 20;  // polynomials: beyond every threshold
            for (int force : {-1, 0, 1}) {
              f.sw.const_sum_rescale_fused = force;
              for (int k = 1; k <= kConstSumRescaleTerms; k++) {
                const ConstSumRescaleRoute r = route_const_sum_rescale(f, nl, big, k, false);
                EXPECT_TRUE(r.rescale.kind == rs.kind && r.rescale.fpmask == rs.fpmask);
                EXPECT_TRUE(r.fused == (can && force != 0));
                EXPECT_TRUE(route_const_sum_rescale(f, nl, 2, k, false).fused == (can && force == 1));  // a tiny batch: only when forced
                EXPECT_TRUE(!route_const_sum_rescale(f, nl, big, k, true).fused);                      // a term above nl: never
                (r.fused ? fused_n : separate_n)++;
              }
              for (int k : {0, kConstSumRescaleTerms + 1, 8, 25}) EXPECT_TRUE(!route_const_sum_rescale(f, nl, big, k, false).fused);
              EQ(csr(f, nl, big), op(f, kRouteRescale, nl) + (can && force != 0 ? " constsum=fused" : " constsum=separate"));
            }
          }
    EXPECT_TRUE(fused_n > 1000 && separate_n > 1000);
  });

  t.run("the measured rule: 64 polynomials and 2^20 coefficients, up to four terms", [&] {
    EXPECT_TRUE(kConstSumRescaleTerms == 4 && kConstSumRescaleMinPolys == 64 && kConstSumRescaleMinCoeffs == ((size_t)1 << 20));
    const RouteFacts f14 = facts(CKKS, 14, FP), f12 = facts(CKKS, 12, FP), f10 = facts(CKKS, 10, FP);
    for (int k = 1; k <= 4; k++) {
      EXPECT_TRUE(route_const_sum_rescale(f14, 4, 64, k, false).fused && !route_const_sum_rescale(f14, 4, 63, k, false).fused);
      EXPECT_TRUE(route_const_sum_rescale(f12, 3, 256, k, false).fused && !route_const_sum_rescale(f12, 3, 255, k, false).fused);  // 2^20 coefficients
      EXPECT_TRUE(!route_const_sum_rescale(facts(CKKS, 16, FP), 3, 4096, k, false).fused);
      EXPECT_TRUE(route_const_sum_rescale(f10, 3, 1024, k, false).fused && !route_const_sum_rescale(f10, 3, 1023, k, false).fused);  // 2^20 coefficients
    }
    EQ(csr(f14, 4, 32), "fp constsum=fused");  // 64 polynomials
    EQ(csr(f14, 4, 31), "fp constsum=separate");
    EQ(csr(facts(CKKS, 10, MIXED), 3, 512), "mixed fpmask=0x6 constsum=fused");
    EQ(csr(facts(CKKS, 15, FP), 3, 4096), "generic constsum=separate");
    RouteFacts nf = facts(CKKS, 12, FP);
    nf.sw.no_fused = true;
    nf.sw.const_sum_rescale_fused = 1;
    EQ(csr(nf, 3, 4096), "generic constsum=separate");
    RouteFacts ni = facts(CKKS, 14, MIXED);
    ni.sw.no_isplit = true;
    ni.sw.const_sum_rescale_fused = 1;
    EQ(csr(ni, 3, 4096), "generic constsum=separate");
  });

  t.run("string 19: the mul_relin route at nl, then the constsum= of the last step", [&] {
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches)
          for (int nl = 2; nl <= (int)bits.size() - 1; nl++)
            for (size_t count : {(size_t)1, (size_t)3, (size_t)128, (size_t)1024}) {
              RouteFacts f = facts(CKKS, logn, bits);
              set(f);
              f.finish();
              EQ(pe(f, nl, count), op(f, kRouteMulRelin, nl, count) + " constsum=separate");
            }
    EQ(pe(facts(CKKS, 10, {50, 30, 30, 30, 30, 30, 30, 50}), 7, 3), "lds_fp constsum=separate");
    EXPECT_TRUE(pe(facts(CKKS, 14, FP), 4, 2).rfind("split14 ", 0) == 0);
  });

  t.run("the op numbers, a short buffer, and format_op keeps the set of operations it had", [&] {
    char b[8];
    const RouteFacts f = facts(CKKS, 14, FP);
    EXPECT_TRUE(kRouteConstSumRescale == 18 && kRoutePolyEval == 19);  // include/abc_hip.h: ABC_HIP_ROUTE_CONST_SUM_RESCALE, _POLY_EVAL
    EXPECT_TRUE(format_const_sum_rescale(b, sizeof b, f, 4, 1) == -1 && format_poly_eval(b, sizeof b, f, 4, 1) == -1);
    char big[160];
    for (int other : {18, 19, 6, 8, 9, 11}) EXPECT_TRUE(format_op(big, sizeof big, f, other, 4, 1, false) == -2);
  });

  t.run("ABC_HIP_NO_CONST_MAC_SUM and ABC_HIP_CONST_SUM_RESCALE_FUSED change no route that existed", [&] {
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (int nl = 2; nl <= (int)bits.size() - 1; nl++) {
          const RouteFacts f = facts(CKKS, logn, bits);
          RouteFacts s = f;
          s.sw.no_const_mac_sum = true;
          s.sw.const_sum_rescale_fused = 1;
          s.finish();
          for (int which : {(int)kRouteMulRelin, (int)kRouteKeyswitch, (int)kRouteRotate, (int)kRouteRescale, (int)kRouteMultiply, (int)kRouteRotateAdd,
                            (int)kRouteRotateMacPlain, (int)kRouteMulPlainRescale, (int)kRouteMulSumRelin})
            for (bool in_place : {false, true}) EQ(op(s, which, nl, 64, in_place), op(f, which, nl, 64, in_place));
          char x[160], y[160];
          EXPECT_TRUE(format_plain_sum_rescale(x, sizeof x, f, nl, 1024) > 0 && format_plain_sum_rescale(y, sizeof y, s, nl, 1024) > 0);
          EQ(x, y);
          EXPECT_TRUE(format_matvec_bsgs(x, sizeof x, f, nl, 64) > 0 && format_matvec_bsgs(y, sizeof y, s, nl, 64) > 0);
          EQ(x, y);
          EXPECT_TRUE(route_plain_mac_sum(s, nl) == route_plain_mac_sum(f, nl));
        }
  });

  return t.summary();
}
