// abc_amd/csrc/abc_route.hpp, route_rotate_mac: where addend + plain (.) rotate(in) becomes three more operands of the key switch's
// last kernel.  Over every (scheme, ring, chain, level, switch set, in_place) tests/cpp/test_route_rotate_add.cpp walks, `fused` is
// true exactly under the rule of DESIGN.md section 3b -- the rotation folds, the sequence is split14 or gsplit15 (nl <= 7), d_out is
// not d_in, ABC_HIP_NO_ROTATE_MAC_FUSION is off -- the strings are the documented ones, and every other route is what it was.
#include <functional>
#include <string>
#include <vector>

#include "../../abc_amd/csrc/abc_route.hpp"
#include "mini_test.hpp"

using namespace abc;
constexpr int BFV = 1, CKKS = 2;

static RouteFacts facts(int scheme, int logn, const std::vector<int> &bits, bool behz_fp = true) {
  RouteFacts f;
  f.scheme = scheme; f.logn = logn; f.K = (int)bits.size(); f.L = f.K - 1; f.nB = f.L; f.behz_fp = behz_fp;
  for (int j = 0; j < f.K; j++) f.bits[j] = (unsigned char)bits[j];
  f.finish();
  return f;
}
static std::vector<int> chain(int first, int mid, int nmid, int special) {
  std::vector<int> b{first};
  b.insert(b.end(), nmid, mid);
  b.push_back(special);
  return b;
}
static std::string op(const RouteFacts &f, int which, int nl, size_t count, bool in_place) {
  char b[128];
  if (format_op(b, sizeof b, f, which, nl, count, in_place) < 0) throw std::runtime_error("format_op failed");
  return b;
}
static std::string rmac(const RouteFacts &f, int nl, size_t count = 1, bool in_place = false) { return op(f, kRouteRotateMacPlain, nl, count, in_place); }
static void eq(const std::string &got, const std::string &want, int line) {
  if (got != want) throw std::runtime_error("line " + std::to_string(line) + ": got \"" + got + "\" want \"" + want + "\"");
}
#define EQ(got, want) eq(got, want, __LINE__)

using Set = std::function<void(RouteFacts &)>;
#define SW(field) Set([](RouteFacts &f) { f.sw.field = true; })

int main() {
  MiniTest t;
  const std::vector<int> HEAD{50, 40, 40, 40, 50};
  const std::vector<Set> switches = {
      Set([](RouteFacts &) {}), SW(no_fused), SW(no_split), SW(no_split4), SW(no_isplit), SW(no_gsplit), SW(no_lean_front), SW(no_bsplit),
      SW(no_mixed), SW(no_pack), SW(no_key_twin), SW(no_bmul), SW(no_iks), SW(no_tensor_intt), SW(no_galois_fusion), SW(main_two_per_cu),
      SW(no_rotate_add_fusion), SW(no_rotate_mac_fusion), Set([](RouteFacts &f) { f.use_fp = false; }), Set([](RouteFacts &f) { f.behz_fp = false; }),
      Set([](RouteFacts &f) { f.sw.lean_limit = 0; }), Set([](RouteFacts &f) { f.sw.no_rotate_mac_fusion = f.sw.no_galois_fusion = true; }),
      Set([](RouteFacts &f) { f.sw.no_rotate_mac_fusion = f.sw.no_split = true; }),
      Set([](RouteFacts &f) { f.sw.no_rotate_add_fusion = f.sw.no_galois_fusion = true; }),
  };
  const std::vector<std::vector<int>> chains = {
      HEAD, {60, 40, 40, 40, 60}, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, chain(48, 48, 8, 49), chain(55, 55, 7, 56), chain(50, 40, 14, 50),
      chain(60, 40, 14, 60), {36, 36, 37}, {60, 40, 40, 60}, chain(50, 40, 13, 50)};

  // Both schemes on every ring 2^10 .. 2^16, chains with every prime fp64-capable and with wider ones, every switch, every level
  t.run("fused exactly under the rule, on a sequence that can, and the string says so", [&] {
    size_t fused_n = 0, separate_n = 0, bfv_n = 0;
    for (int scheme : {BFV, CKKS})
      for (int logn = 10; logn <= 16; logn++)
        for (const std::vector<int> &bits : chains)
          for (bool behz_fp : {true, false})
            for (const Set &set : switches)
              for (int nl = 1; nl <= (int)bits.size() - 1; nl++)
                for (bool in_place : {false, true}) {
                  RouteFacts f = facts(scheme, logn, bits, behz_fp);
                  set(f);
                  f.finish();
                  const RotMacRoute r = route_rotate_mac(f, nl, in_place);
                  // the rotation is the out-of-place one whatever d_out is: the unfused sequence rotates into an arena
                  const RotRoute rot = route_rotate(f, nl, false);
                  EXPECT_TRUE(r.rot.fold == rot.fold && r.rot.ks.seq == rot.ks.seq && r.rot.ks.front == rot.ks.front);
                  const Seq q = rot.ks.seq;
                  const bool seq_ok = q == Seq::split14 || (q == Seq::gsplit15 && nl <= 7);
                  EXPECT_TRUE(seq_takes_plain(f, rot.ks, nl) == seq_ok);
                  const bool want = rot.fold && seq_ok && !in_place && !f.sw.no_rotate_mac_fusion;
                  EXPECT_TRUE(r.fused == want);
                  // what the launch checks (launch_keyswitch): a plaintext goes to a folding sequence that takes one; those take acc too
                  if (r.fused) EXPECT_TRUE(seq_folds_permutation(f, r.rot.ks) && seq_takes_acc(f, r.rot.ks, nl));
                  if (scheme == BFV) {  // the call itself refuses a BFV context
                    EXPECT_TRUE(!r.fused);
                    bfv_n++;
                  }
                  (want ? fused_n : separate_n)++;
                  for (size_t count : {(size_t)1, (size_t)512}) {
                    const std::string rs = op(f, kRouteRotate, nl, count, false), got = rmac(f, nl, count, in_place);
                    const size_t sp = rs.find(' ');
                    const std::string head = rs.substr(0, sp), ks = rs.substr(sp + 1);  // "fold" / "permute", the key switch
                    EQ(got, want ? "fold+mac " + ks : head + " mac=separate " + ks);
                  }
                }
    EXPECT_TRUE(fused_n > 1000 && separate_n > 1000 && bfv_n > 1000);
  });

  t.run("the documented strings", [&] {
    const RouteFacts f = facts(CKKS, 14, HEAD);
    EQ(rmac(f, 4), "fold+mac split14 front=lean pack=1 main=split4");
    EQ(rmac(f, 4, 8192), "fold+mac split14 front=fat pack=1 main=split4");
    EQ(rmac(f, 4, 1, true), "fold mac=separate split14 front=lean pack=1 main=split4");
    RouteFacts g = f;
    g.sw.no_rotate_mac_fusion = true;
    EQ(rmac(g, 4), "fold mac=separate split14 front=lean pack=1 main=split4");
    g = f;
    g.sw.no_rotate_add_fusion = true;  // the other call's switch
    EQ(rmac(g, 4), "fold+mac split14 front=lean pack=1 main=split4");
    g = f;
    g.sw.no_galois_fusion = true;
    EQ(rmac(g, 4), "permute mac=separate split14 front=lean pack=1 main=split4");
    g = f;
    g.sw.no_split = true;
    EQ(rmac(g, 4), "permute mac=separate lds_fp");
    g = f;
    g.sw.no_fused = true;
    EQ(rmac(g, 4), "permute mac=separate generic front=plain");
    g = f;
    g.sw.no_split4 = true;
    EQ(rmac(g, 4), "fold+mac split14 front=lean pack=0 main=split3");
    const RouteFacts deep = facts(CKKS, 14, chain(50, 40, 13, 50));
    EQ(rmac(deep, 5), "fold+mac split14 front=lean pack=1 main=split4");
    EQ(rmac(deep, 6), "fold+mac split14 front=lean pack=0 main=split3");
    EQ(rmac(deep, 12), "fold+mac split14 front=lean pack=0 main=split3");
    EQ(rmac(deep, 13), "permute mac=separate lds_fp");
    EQ(rmac(facts(CKKS, 14, {60, 40, 40, 60}), 3), "fold mac=separate isplit14 guard=1 fpmask=0x6");
    const RouteFacts f15 = facts(CKKS, 15, chain(50, 40, 14, 50));
    EQ(rmac(f15, 3), "fold+mac gsplit15");
    EQ(rmac(f15, 7), "fold+mac gsplit15");
    EQ(rmac(f15, 8), "fold mac=separate gsplit15");  // k_gsplit_main_deep takes no plaintext
    EQ(rmac(f15, 3, 1, true), "fold mac=separate gsplit15");
    EQ(rmac(facts(CKKS, 15, {60, 40, 40, 60}), 3), "fold mac=separate isplit15 guard=1 fpmask=0x6");
    EQ(rmac(facts(CKKS, 13, HEAD), 4), "permute mac=separate lds_fp");
    EQ(rmac(facts(CKKS, 16, HEAD), 4), "permute mac=separate generic front=fp");
    // a BFV context is refused by the call; the table only never fuses there
    EQ(rmac(facts(BFV, 14, {48, 48, 48, 49, 49, 49, 49, 49, 49}), 8), "fold mac=separate bsplit14 pass0=per_target");
    EQ(rmac(facts(BFV, 13, {43, 43, 44, 44, 44}), 4), "fold mac=separate bsplit_big");
  });

  t.run("every other route gives the string it gave, under the new switch too", [&] {
    for (bool sw : {false, true}) {
      RouteFacts f = facts(CKKS, 14, HEAD);
      f.sw.no_rotate_mac_fusion = sw;
      EQ(op(f, kRouteRotateAdd, 4, 1, false), "fold+add split14 front=lean pack=1 main=split4");
      EQ(op(f, kRouteRotateAdd, 4, 1, true), "fold add=separate split14 front=lean pack=1 main=split4");
      EQ(op(f, kRouteRotate, 4, 1, false), "fold split14 front=lean pack=1 main=split4");
      EQ(op(f, kRouteRotate, 4, 1, true), "permute split14 front=lean pack=1 main=split4");
      EQ(op(f, kRouteMulRelin, 4, 1, false), "split14 front=lean pack=1 main=split4");
      EQ(op(f, kRouteKeyswitch, 4, 8192, false), "split14 front=fat pack=1 main=split4");
      EQ(op(f, kRouteRescale, 4, 1, false), "fp");
      EQ(op(f, kRouteMultiply, 4, 1, false), "tensor");
      RouteFacts f15 = facts(CKKS, 15, chain(50, 40, 14, 50));
      f15.sw.no_rotate_mac_fusion = sw;
      EQ(op(f15, kRouteRotateAdd, 7, 1, false), "fold+add gsplit15");
      EQ(op(f15, kRouteRotateAdd, 8, 1, false), "fold add=separate gsplit15");
      RouteFacts b = facts(BFV, 14, {48, 48, 48, 49, 49, 49, 49, 49, 49});
      b.sw.no_rotate_mac_fusion = sw;
      EQ(op(b, kRouteRotateAdd, 8, 1, false), "fold+add bsplit14 pass0=per_target");
      EQ(op(b, kRouteMulRelin, 8, 1, false), "bmul");
    }
    // with the new switch off and on, every operation that existed formats alike on every shape
    for (int scheme : {BFV, CKKS})
      for (int logn = 10; logn <= 16; logn++)
        for (const std::vector<int> &bits : chains)
          for (int nl = (scheme == BFV ? (int)bits.size() - 1 : 1); nl <= (int)bits.size() - 1; nl++)
            for (int which : {(int)kRouteMulRelin, (int)kRouteKeyswitch, (int)kRouteRotate, (int)kRouteMultiply, (int)kRouteRotateAdd})
              for (bool in_place : {false, true}) {
                RouteFacts f = facts(scheme, logn, bits), g = f;
                g.sw.no_rotate_mac_fusion = true;
                EQ(op(g, which, nl, 64, in_place), op(f, which, nl, 64, in_place));
              }
  });

  t.run("short buffer, unknown operations", [&] {
    char b[64];
    volatile size_t cap = 8;
    const RouteFacts f = facts(CKKS, 14, HEAD);
    EXPECT_TRUE(kRouteRotateMacPlain == 7);  // include/abc_hip.h: ABC_HIP_ROUTE_ROTATE_MAC_PLAIN
    EXPECT_TRUE(format_op(b, cap, f, kRouteRotateMacPlain, 4, 1, false) == -1);
    EXPECT_TRUE(format_op(b, sizeof b, f, 6, 4, 1, false) == -2);  // unassigned
    EXPECT_TRUE(format_op(b, sizeof b, f, 8, 4, 1, false) == -2);
  });
  return t.summary();
}
