// abc_amd/csrc/abc_route.hpp, route_rotate_add: where addend + rotate(in) becomes one more operand of the key switch's last kernel.
// Over every (scheme, ring, chain, level, switch set, in_place) tests/cpp/test_route.cpp names, `fused` is true exactly under the
// rule of DESIGN.md section 3b -- the rotation folds, the sequence is split14 / gsplit15 (nl <= 7) / bsplit14 / bsplit_big, d_out
// is not d_in, ABC_HIP_NO_ROTATE_ADD_FUSION is off -- and the strings are the documented ones.
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
static std::string radd(const RouteFacts &f, int nl, size_t count = 1, bool in_place = false) { return op(f, kRouteRotateAdd, nl, count, in_place); }
static void eq(const std::string &got, const std::string &want, int line) {
  if (got != want) throw std::runtime_error("line " + std::to_string(line) + ": got \"" + got + "\" want \"" + want + "\"");
}
#define EQ(got, want) eq(got, want, __LINE__)

using Set = std::function<void(RouteFacts &)>;
#define SW(field) Set([](RouteFacts &f) { f.sw.field = true; })

int main() {
  MiniTest t;
  const std::vector<int> HEAD{50, 40, 40, 40, 50};

  // every chain of test_route.cpp, BFV rings at their top level and CKKS at every level
  struct Shape { int scheme, logn; std::vector<int> bits; bool behz_fp; };
  std::vector<Shape> shapes = {
      {CKKS, 14, HEAD, true}, {CKKS, 14, {60, 40, 40, 40, 60}, true}, {CKKS, 14, {60, 40, 40, 60}, true}, {CKKS, 14, {57, 45, 45, 57}, true},
      {CKKS, 14, {55, 52, 51, 55}, true}, {CKKS, 14, {60, 50, 40, 50}, true}, {CKKS, 14, {50, 40, 58, 40, 50}, true},
      {CKKS, 14, chain(60, 40, 4, 60), true}, {CKKS, 14, chain(60, 45, 6, 60), true}, {CKKS, 14, chain(50, 40, 6, 50), true},
      {CKKS, 14, {50, 46, 46, 46, 50}, true}, {CKKS, 14, {48, 40, 44, 36, 49}, true}, {CKKS, 14, {41, 40, 48, 49, 50, 47}, true},
      {CKKS, 14, chain(50, 40, 13, 50), true}, {CKKS, 14, chain(50, 40, 14, 50), true}, {CKKS, 14, chain(60, 40, 8, 60), true},
      {CKKS, 14, {50, 40, 40, 51}, true}, {CKKS, 14, {51, 40, 40, 50}, true}, {CKKS, 14, {61, 40, 40, 60}, true},
      {CKKS, 13, HEAD, true}, {CKKS, 16, HEAD, true},
      {CKKS, 15, {50, 40, 40, 50}, true}, {CKKS, 15, {60, 40, 40, 60}, true}, {CKKS, 15, chain(50, 40, 14, 50), true},
      {CKKS, 15, chain(50, 40, 15, 50), true}, {CKKS, 15, chain(60, 40, 14, 60), true}, {CKKS, 15, {61, 40, 40, 60}, true},
      {BFV, 12, {36, 36, 37}, true}, {BFV, 13, {43, 43, 44, 44, 44}, true}, {BFV, 14, {48, 48, 48, 49, 49, 49, 49, 49, 49}, true},
      {BFV, 15, chain(55, 55, 14, 56), false}, {BFV, 16, chain(55, 55, 7, 56), false}, {BFV, 16, chain(49, 49, 7, 50), true},
      {BFV, 14, chain(48, 48, 7, 49), true}, {BFV, 14, chain(48, 48, 8, 49), true}, {BFV, 13, chain(48, 48, 7, 49), true},
      {BFV, 13, chain(48, 48, 8, 49), true}, {BFV, 16, chain(48, 48, 8, 49), true}, {BFV, 14, chain(48, 48, 7, 50), true},
      {BFV, 14, chain(48, 48, 7, 51), true}, {BFV, 15, chain(49, 49, 7, 50), true},
  };
  const std::vector<Set> switches = {
      Set([](RouteFacts &) {}), SW(no_fused), SW(no_split), SW(no_split4), SW(no_isplit), SW(no_gsplit), SW(no_lean_front), SW(no_bsplit),
      SW(no_mixed), SW(no_pack), SW(no_key_twin), SW(no_bmul), SW(no_iks), SW(no_tensor_intt), SW(no_galois_fusion), SW(main_two_per_cu),
      SW(no_rotate_add_fusion), Set([](RouteFacts &f) { f.use_fp = false; }), Set([](RouteFacts &f) { f.behz_fp = false; }),
      Set([](RouteFacts &f) { f.sw.lean_limit = 0; }), Set([](RouteFacts &f) { f.sw.no_rotate_add_fusion = f.sw.no_galois_fusion = true; }),
      Set([](RouteFacts &f) { f.sw.no_rotate_add_fusion = f.sw.no_split = true; }),
  };

  t.run("fused exactly under the rule, and the string says so", [&] {
    size_t fused_n = 0, separate_n = 0;
    for (const Shape &s : shapes)
      for (const Set &set : switches)
        for (int nl = (s.scheme == BFV ? (int)s.bits.size() - 1 : 1); nl <= (int)s.bits.size() - 1; nl++)
          for (bool in_place : {false, true})
            for (size_t count : {(size_t)1, (size_t)512}) {
              RouteFacts f = facts(s.scheme, s.logn, s.bits, s.behz_fp);
              set(f);
              f.finish();
              const RotAddRoute r = route_rotate_add(f, nl, in_place);
              // the rotation is the out-of-place one whatever d_out is: the unfused sequence rotates into an arena
              const RotRoute rot = route_rotate(f, nl, false);
              EXPECT_TRUE(r.rot.fold == rot.fold && r.rot.ks.seq == rot.ks.seq && r.rot.ks.front == rot.ks.front);
              const Seq q = rot.ks.seq;
              const bool seq_ok = q == Seq::split14 || q == Seq::bsplit14 || q == Seq::bsplit_big || (q == Seq::gsplit15 && nl <= 7);
              const bool want = rot.fold && seq_ok && !in_place && !f.sw.no_rotate_add_fusion;
              EXPECT_TRUE(r.fused == want);
              (want ? fused_n : separate_n)++;
              const std::string rs = op(f, kRouteRotate, nl, count, false), got = radd(f, nl, count, in_place);
              const size_t sp = rs.find(' ');
              const std::string head = rs.substr(0, sp), ks = rs.substr(sp + 1);  // "fold" / "permute", the key switch
              EQ(got, want ? "fold+add " + ks : head + " add=separate " + ks);
            }
    EXPECT_TRUE(fused_n > 100 && separate_n > 100);
  });

  // The launch code checks a call against seq_folds_permutation / seq_takes_acc (launch_keyswitch) and nothing else: a route that
  // folds or fuses must name a sequence that can.  Both schemes on every ring 2^10 .. 2^16, chains with every prime fp64-capable and
  // with wider ones, every switch, every level.
  t.run("a route folds / fuses only where the sequence can; fused is the old expression", [&] {
    const std::vector<std::vector<int>> chains = {
        HEAD, {60, 40, 40, 40, 60}, {55, 52, 51, 55}, {50, 40, 58, 40, 50}, chain(48, 48, 8, 49), chain(55, 55, 7, 56), chain(50, 40, 14, 50),
        chain(60, 40, 14, 60), {36, 36, 37}};
    size_t folds = 0, fused_n = 0, total = 0;
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
                  const RotRoute rot = route_rotate(f, nl, in_place);
                  if (rot.fold) EXPECT_TRUE(seq_folds_permutation(f, rot.ks));
                  const RotAddRoute r = route_rotate_add(f, nl, in_place);
                  if (r.fused) EXPECT_TRUE(r.rot.fold && seq_folds_permutation(f, r.rot.ks) && seq_takes_acc(f, r.rot.ks, nl));
                  // what route_rotate_add computed before the predicates existed, word for word
                  const Seq s = r.rot.ks.seq;
                  const bool takes_acc = s == Seq::split14 || s == Seq::bsplit14 || s == Seq::bsplit_big || (s == Seq::gsplit15 && nl <= 7);
                  EXPECT_TRUE(r.fused == (r.rot.fold && takes_acc && !in_place && !f.sw.no_rotate_add_fusion));
                  EXPECT_TRUE(seq_takes_acc(f, r.rot.ks, nl) == takes_acc);
                  folds += rot.fold;
                  fused_n += r.fused;
                  total++;
                }
    EXPECT_TRUE(folds > 1000 && fused_n > 1000 && total - folds > 1000);
  });

  t.run("the documented strings", [&] {
    const RouteFacts f = facts(CKKS, 14, HEAD);
    EQ(radd(f, 4), "fold+add split14 front=lean pack=1 main=split4");
    EQ(radd(f, 4, 8192), "fold+add split14 front=fat pack=1 main=split4");
    EQ(radd(f, 4, 1, true), "fold add=separate split14 front=lean pack=1 main=split4");
    RouteFacts g = f;
    g.sw.no_rotate_add_fusion = true;
    EQ(radd(g, 4), "fold add=separate split14 front=lean pack=1 main=split4");
    g = f;
    g.sw.no_galois_fusion = true;
    EQ(radd(g, 4), "permute add=separate split14 front=lean pack=1 main=split4");
    g = f;
    g.sw.no_split = true;
    EQ(radd(g, 4), "permute add=separate lds_fp");
    g = f;
    g.sw.no_fused = true;
    EQ(radd(g, 4), "permute add=separate generic front=plain");
    g = f;
    g.sw.no_split4 = true;
    EQ(radd(g, 4), "fold+add split14 front=lean pack=0 main=split3");
    const RouteFacts deep = facts(CKKS, 14, chain(50, 40, 13, 50));
    EQ(radd(deep, 5), "fold+add split14 front=lean pack=1 main=split4");
    EQ(radd(deep, 6), "fold+add split14 front=lean pack=0 main=split3");
    EQ(radd(deep, 12), "fold+add split14 front=lean pack=0 main=split3");
    EQ(radd(deep, 13), "permute add=separate lds_fp");
    EQ(radd(facts(CKKS, 14, {60, 40, 40, 60}), 3), "fold add=separate isplit14 guard=1 fpmask=0x6");
    const RouteFacts f15 = facts(CKKS, 15, chain(50, 40, 14, 50));
    EQ(radd(f15, 3), "fold+add gsplit15");
    EQ(radd(f15, 7), "fold+add gsplit15");
    EQ(radd(f15, 8), "fold add=separate gsplit15");  // k_gsplit_main_deep takes no second addend
    EQ(radd(f15, 3, 1, true), "fold add=separate gsplit15");
    EQ(radd(facts(CKKS, 15, {60, 40, 40, 60}), 3), "fold add=separate isplit15 guard=1 fpmask=0x6");
    EQ(radd(facts(BFV, 12, {36, 36, 37}), 2), "permute add=separate lds_fp");
    EQ(radd(facts(BFV, 13, {43, 43, 44, 44, 44}), 4), "fold+add bsplit_big");
    const RouteFacts b14 = facts(BFV, 14, {48, 48, 48, 49, 49, 49, 49, 49, 49});
    EQ(radd(b14, 8), "fold+add bsplit14 pass0=per_target");
    EQ(radd(b14, 8, 40), "fold+add bsplit14 pass0=per_limb");
    EQ(radd(facts(BFV, 16, chain(49, 49, 7, 50)), 8), "fold+add bsplit_big");
    EQ(radd(facts(BFV, 16, chain(55, 55, 7, 56), false), 8), "fold add=separate generic front=iks guard=0");
  });

  t.run("short buffer; the other operations are untouched by the new switch", [&] {
    char b[64];
    volatile size_t cap = 8;
    RouteFacts f = facts(CKKS, 14, HEAD);
    EXPECT_TRUE(format_op(b, cap, f, kRouteRotateAdd, 4, 1, false) == -1);
    EXPECT_TRUE(format_op(b, sizeof b, f, 6, 4, 1, false) == -2);
    f.sw.no_rotate_add_fusion = true;
    EQ(op(f, kRouteRotate, 4, 1, false), "fold split14 front=lean pack=1 main=split4");
    EQ(op(f, kRouteMulRelin, 4, 1, false), "split14 front=lean pack=1 main=split4");
  });
  return t.summary();
}
