// abc_amd/csrc/abc_route.hpp, route_mulplain_rescale: where rescale(ct (.) plain) forms the product in the rescale's own loads.
// Over every ring 2^10 .. 2^16, chains whose primes are all fp64-capable, mixed and 60-bit ones, every level and every switch, `fused`
// is true exactly where route_rescale (out of place) gives the LDS-resident kernels -- fp or mixed -- and
// ABC_HIP_NO_MULPLAIN_RESCALE_FUSION is off; the string is the rescale's plus " mulplain=fused" / " mulplain=separate", and every other
// route is what it was.  No shape is sent to the separate route by measurement: profiles/mulplain_rescale_ab.log has the fused
// median at or below the separate one at every shape measured (N = 2^14 and 2^12, batches 32 .. 1024), so the rule has no threshold.
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
static std::string mpr(const RouteFacts &f, int nl, size_t count = 1) { return op(f, kRouteMulPlainRescale, nl, count); }
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
      Set([](RouteFacts &f) { f.sw.no_mulplain_rescale_fusion = f.sw.no_fused = true; }),
      Set([](RouteFacts &f) { f.sw.no_mulplain_rescale_fusion = f.sw.no_mixed = true; }),
  };
  const std::vector<std::vector<int>> chains = {FP, MIXED, WIDE, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, {50, 40, 50}, {36, 36, 37}, {50, 50, 50, 50}};

  t.run("fused exactly on the LDS-resident rescale, and the string says so", [&] {
    size_t fused_n = 0, separate_n = 0;
    for (int logn = 10; logn <= 16; logn++)
      for (const std::vector<int> &bits : chains)
        for (const Set &set : switches)
          for (int nl = 2; nl <= (int)bits.size() - 1; nl++) {
            RouteFacts f = facts(CKKS, logn, bits);
            set(f);
            f.finish();
            const MulPlainRescaleRoute r = route_mulplain_rescale(f, nl);
            const RescaleRoute rs = route_rescale(f, nl, false);
            EXPECT_TRUE(r.rescale.kind == rs.kind && r.rescale.fpmask == rs.fpmask);
            // the rule, spelt out: a ring that fits LDS, not ABC_HIP_NO_FUSED, and with a prime above 2^50 (or fp64 off) not
            // ABC_HIP_NO_ISPLIT; then the new switch
            const bool lds = logn >= 10 && logn <= 14 && !f.sw.no_fused && ((f.use_fp && f.data_fp(nl)) || !f.sw.no_isplit);
            EXPECT_TRUE((rs.kind != Rescale::generic) == lds);
            const bool want = lds && !f.sw.no_mulplain_rescale_fusion;
            EXPECT_TRUE(r.fused == want);
            (want ? fused_n : separate_n)++;
            for (size_t count : {(size_t)1, (size_t)32, (size_t)1024})  // no threshold in the batch: profiles/mulplain_rescale_ab.log
              EQ(mpr(f, nl, count), op(f, kRouteRescale, nl, count) + (want ? " mulplain=fused" : " mulplain=separate"));
          }
    EXPECT_TRUE(fused_n > 500 && separate_n > 500);
  });

  t.run("the documented strings", [&] {
    for (int logn = 10; logn <= 14; logn++) {
      EQ(mpr(facts(CKKS, logn, FP), 4), "fp mulplain=fused");
      EQ(mpr(facts(CKKS, logn, FP), 2), "fp mulplain=fused");
      EQ(mpr(facts(CKKS, logn, MIXED), 3), "mixed fpmask=0x6 mulplain=fused");
      EQ(mpr(facts(CKKS, logn, MIXED), 2), "mixed fpmask=0x2 mulplain=fused");
      EQ(mpr(facts(CKKS, logn, WIDE), 3), "mixed fpmask=0x0 mulplain=fused");
    }
    for (int logn : {15, 16})
      for (const std::vector<int> &bits : {FP, MIXED, WIDE}) EQ(mpr(facts(CKKS, logn, bits), 3), "generic mulplain=separate");
    RouteFacts g = facts(CKKS, 12, FP);
    g.sw.no_fused = true;
    EQ(mpr(g, 4), "generic mulplain=separate");
    g = facts(CKKS, 12, FP);
    g.sw.no_mulplain_rescale_fusion = true;
    EQ(mpr(g, 4), "fp mulplain=separate");
    g = facts(CKKS, 12, MIXED);
    g.sw.no_mulplain_rescale_fusion = true;
    EQ(mpr(g, 3), "mixed fpmask=0x6 mulplain=separate");
    g = facts(CKKS, 12, MIXED);
    g.sw.no_mixed = true;
    EQ(mpr(g, 3), "mixed fpmask=0x0 mulplain=fused");
    g = facts(CKKS, 14, MIXED);
    g.sw.no_isplit = true;
    EQ(mpr(g, 3), "generic mulplain=separate");
    g = facts(CKKS, 14, FP);
    g.sw.no_isplit = true;  // no prime above 2^50: the switch has nothing to say
    EQ(mpr(g, 4), "fp mulplain=fused");
    g = facts(CKKS, 14, FP);
    g.use_fp = false;
    g.finish();
    EQ(mpr(g, 4), "mixed fpmask=0x0 mulplain=fused");
  });

  t.run("every other route gives the string it gave, under the new switch too", [&] {
    for (int scheme : {BFV, CKKS})
      for (int logn = 10; logn <= 16; logn++)
        for (const std::vector<int> &bits : chains)
          for (int nl = (scheme == BFV ? (int)bits.size() - 1 : 1); nl <= (int)bits.size() - 1; nl++)
            for (int which : {(int)kRouteMulRelin, (int)kRouteKeyswitch, (int)kRouteRotate, (int)kRouteRescale, (int)kRouteMultiply, (int)kRouteRotateAdd,
                              (int)kRouteRotateMacPlain})
              for (bool in_place : {false, true}) {
                if (which == kRouteRescale && (scheme == BFV || nl < 2)) continue;
                RouteFacts f = facts(scheme, logn, bits), g = f;
                g.sw.no_mulplain_rescale_fusion = true;
                EQ(op(g, which, nl, 64, in_place), op(f, which, nl, 64, in_place));
              }
    const RouteFacts f = facts(CKKS, 14, FP);
    EQ(op(f, kRouteRescale, 4), "fp");
    EQ(op(f, kRouteRescale, 4, 1, true), "generic");
    EQ(op(f, kRouteRotateMacPlain, 4), "fold+mac split14 front=lean pack=1 main=split4");
  });

  t.run("the op numbers, a short buffer, unknown operations", [&] {
    char b[64];
    volatile size_t cap = 8;
    const RouteFacts f = facts(CKKS, 14, FP);
    EXPECT_TRUE(kRouteMulPlainRescale == 10);  // include/abc_hip.h: ABC_HIP_ROUTE_MULTIPLY_PLAIN_RESCALE
    EXPECT_TRUE(format_op(b, cap, f, kRouteMulPlainRescale, 4, 1, false) == -1);
    for (int unassigned : {6, 8, 9, 11})  // 6, 8 and 9: what the other route tests probe as the unknown operation
      EXPECT_TRUE(format_op(b, sizeof b, f, unassigned, 4, 1, false) == -2);
    EXPECT_TRUE(format_op(b, sizeof b, f, -1, 4, 1, false) == -2);
  });
  return t.summary();
}
