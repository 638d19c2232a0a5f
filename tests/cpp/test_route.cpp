// abc_amd/csrc/abc_route.hpp on hand-made facts: the route string of every configuration the repository names (with no switch and
// with each switch that can affect it), of every boundary in the table, and the questions the dispatchers used to answer twice.
// The expected strings are today's behaviour, asymmetries included (DESIGN.md section 3b lists them).
#include <initializer_list>
#include <string>
#include <vector>

#include "../../abc_amd/csrc/abc_route.hpp"
#include "mini_test.hpp"

using namespace abc;
constexpr int BFV = 1, CKKS = 2;

// key chain `bits` (last: the special prime); BFV defaults to the nB == L of the BFVDefault shapes
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
template <class Fn>
static RouteFacts with(RouteFacts f, Fn set) {
  set(f);
  f.finish();
  return f;
}
#define SW(field) [](RouteFacts &f) { f.sw.field = true; }
static const auto NO_FP64 = [](RouteFacts &f) { f.use_fp = false; };
static const auto BEHZ_INT = [](RouteFacts &f) { f.behz_fp = false; };

static std::string op(const RouteFacts &f, int which, int nl, size_t count, bool in_place) {
  char b[128];
  if (format_op(b, sizeof b, f, which, nl, count, in_place) < 0) throw std::runtime_error("format_op failed");
  return b;
}
static std::string mul(const RouteFacts &f, int nl, size_t count = 1) { return op(f, kRouteMulRelin, nl, count, false); }
static std::string ks(const RouteFacts &f, int nl, size_t count = 1) { return op(f, kRouteKeyswitch, nl, count, false); }
static std::string rot(const RouteFacts &f, int nl, size_t count = 1, bool in_place = false) { return op(f, kRouteRotate, nl, count, in_place); }
static std::string resc(const RouteFacts &f, int nl, bool in_place = false) { return op(f, kRouteRescale, nl, 1, in_place); }
static std::string bmul(const RouteFacts &f) { return op(f, kRouteMultiply, f.L, 1, false); }
static void eq(const std::string &got, const std::string &want, int line) {
  if (got != want) throw std::runtime_error("line " + std::to_string(line) + ": got \"" + got + "\" want \"" + want + "\"");
}
#define EQ(got, want) eq(got, want, __LINE__)

int main() {
  MiniTest t;
  const std::vector<int> HEAD{50, 40, 40, 40, 50}, B60{60, 40, 40, 40, 60};

  t.run("bench.py headline chain, N = 2^14, each switch", [&] {
    const RouteFacts f = facts(CKKS, 14, HEAD);
    EQ(mul(f, 4), "split14 front=lean pack=1 main=split4");
    EQ(mul(f, 4, 8192), "split14 front=fat pack=1 main=split4");  // chunks of 128: 512 (ciphertext, limb) pairs
    EQ(ks(f, 4), "split14 front=lean pack=1 main=split4");
    EQ(rot(f, 4), "fold split14 front=lean pack=1 main=split4");
    EQ(rot(f, 4, 1, true), "permute split14 front=lean pack=1 main=split4");
    EQ(resc(f, 4), "fp");
    EQ(resc(f, 4, true), "generic");
    EQ(mul(with(f, SW(no_lean_front)), 4), "split14 front=fat pack=1 main=split4");
    EQ(mul(with(f, SW(no_pack)), 4), "split14 front=lean pack=0 main=split4");
    EQ(mul(with(f, SW(no_split4)), 4), "split14 front=lean pack=0 main=split3");
    EQ(mul(with(f, SW(no_split)), 4), "lds_fp");
    EQ(rot(with(f, SW(no_split)), 4), "permute lds_fp");
    EQ(mul(with(f, SW(no_fused)), 4), "generic mul=tensor ks=generic front=plain");
    EQ(rot(with(f, SW(no_fused)), 4), "permute generic front=plain");
    EQ(resc(with(f, SW(no_fused)), 4), "generic");
    EQ(mul(with(f, NO_FP64), 4), "isplit14 guard=0 fpmask=0x0");
    EQ(rot(with(f, NO_FP64), 4), "fold isplit14 guard=0 fpmask=0x0");
    EQ(resc(with(f, NO_FP64), 4), "mixed fpmask=0x0");
    EQ(mul(with(with(f, NO_FP64), SW(no_isplit)), 4), "lds_int guard=0 lazy=1");
    EQ(rot(with(with(f, NO_FP64), SW(no_isplit)), 4), "permute lds_int guard=0 lazy=1");
    EQ(resc(with(with(f, NO_FP64), SW(no_isplit)), 4), "generic");
    EQ(rot(with(f, SW(no_galois_fusion)), 4), "permute split14 front=lean pack=1 main=split4");
    for (auto set : {+SW(no_isplit), +SW(no_gsplit), +SW(no_bsplit), +SW(no_mixed), +SW(no_key_twin), +SW(no_bmul), +SW(no_iks), +SW(no_tensor_intt)})
      EQ(mul(with(f, set), 4), "split14 front=lean pack=1 main=split4");
  });

  t.run("bench.py 60-bit chain and WIDE_CHAINS, N = 2^14", [&] {
    const RouteFacts f = facts(CKKS, 14, B60);
    EQ(mul(f, 4), "isplit14 guard=1 fpmask=0xe");
    EQ(rot(f, 4), "fold isplit14 guard=1 fpmask=0xe");
    EQ(resc(f, 4), "mixed fpmask=0xe");
    EQ(resc(f, 2), "mixed fpmask=0x2");
    EQ(mul(with(f, SW(no_mixed)), 4), "isplit14 guard=1 fpmask=0x0");
    EQ(resc(with(f, SW(no_mixed)), 4), "mixed fpmask=0x0");
    EQ(mul(with(f, NO_FP64), 4), "isplit14 guard=1 fpmask=0x0");
    EQ(mul(with(f, SW(no_isplit)), 4), "lds_int guard=1 lazy=0");
    EQ(resc(with(f, SW(no_isplit)), 4), "generic");
    EQ(mul(with(f, SW(no_split)), 4), "lds_int guard=1 lazy=0");
    EQ(mul(with(f, SW(no_fused)), 4), "generic mul=tensor ks=generic front=plain");
    EQ(rot(with(f, SW(no_galois_fusion)), 4), "permute isplit14 guard=1 fpmask=0xe");
    EQ(mul(facts(CKKS, 14, {60, 40, 40, 60}), 3), "isplit14 guard=1 fpmask=0x6");
    EQ(mul(facts(CKKS, 14, {57, 45, 45, 57}), 3), "isplit14 guard=0 fpmask=0x6");
    EQ(mul(with(facts(CKKS, 14, {57, 45, 45, 57}), SW(no_isplit)), 3), "lds_int guard=0 lazy=0");
    EQ(mul(facts(CKKS, 14, {55, 52, 51, 55}), 3), "isplit14 guard=0 fpmask=0x0");
    EQ(mul(with(facts(CKKS, 14, {55, 52, 51, 55}), SW(no_isplit)), 3), "lds_int guard=0 lazy=1");
    EQ(mul(facts(CKKS, 14, {60, 50, 40, 50}), 3), "isplit14 guard=1 fpmask=0x6");
    EQ(mul(facts(CKKS, 14, {50, 40, 58, 40, 50}), 4), "isplit14 guard=1 fpmask=0xb");
    EQ(resc(facts(CKKS, 14, {50, 40, 58, 40, 50}), 2), "fp");  // the two limbs left of the wide prime
    EQ(mul(facts(CKKS, 14, chain(60, 40, 4, 60)), 5), "isplit14 guard=1 fpmask=0x1e");
    EQ(mul(facts(CKKS, 14, chain(60, 45, 6, 60)), 7), "isplit14 guard=1 fpmask=0x7e");
    EQ(mul(facts(CKKS, 14, chain(50, 40, 6, 50)), 7), "split14 front=lean pack=0 main=split3");
    EQ(mul(facts(CKKS, 14, chain(50, 40, 6, 50)), 1), "split14 front=lean pack=1 main=split4");
  });

  t.run("PACK_CHAINS, lean and fat front", [&] {
    for (const std::vector<int> &b : {std::vector<int>{50, 46, 46, 46, 50}, {48, 40, 44, 36, 49}, {41, 40, 48, 49, 50, 47}}) {
      const RouteFacts f = facts(CKKS, 14, b);
      for (int nl = 1; nl <= f.L; nl++) {
        EQ(mul(f, nl, 5), "split14 front=lean pack=1 main=split4");
        EQ(mul(with(f, SW(no_lean_front)), nl, 5), "split14 front=fat pack=1 main=split4");
        EQ(rot(f, nl), "fold split14 front=lean pack=1 main=split4");
      }
    }
  });

  t.run("BFVDefault 4096 / 8192 / 16384 / 32768", [&] {
    const RouteFacts f12 = facts(BFV, 12, {36, 36, 37});
    EQ(mul(f12, 2), "generic mul=behz ks=lds_fp");
    EQ(rot(f12, 2), "permute lds_fp");
    EQ(bmul(f12), "behz");
    EQ(mul(with(f12, NO_FP64), 2), "generic mul=behz ks=lds_int guard=0 lazy=1");
    EQ(mul(with(f12, SW(no_fused)), 2), "generic mul=behz ks=generic front=plain");

    const RouteFacts f13 = facts(BFV, 13, {43, 43, 44, 44, 44});
    EQ(mul(f13, 4), "bmul");
    EQ(ks(f13, 4), "bsplit_big");
    EQ(rot(f13, 4), "fold bsplit_big");
    EQ(rot(f13, 4, 1, true), "permute bsplit_big");
    EQ(bmul(f13), "bmul_big");
    EQ(mul(with(f13, SW(no_bmul)), 4), "generic mul=behz ks=bsplit_big");
    EQ(mul(with(f13, SW(no_bsplit)), 4), "generic mul=bmul_big ks=lds_fp");
    EQ(rot(with(f13, SW(no_bsplit)), 4), "permute lds_fp");
    EQ(mul(with(f13, SW(no_gsplit)), 4), "generic mul=bmul_big ks=lds_fp");  // the 2^15 switch also turns this ring's split key switch off
    EQ(mul(with(f13, BEHZ_INT), 4), "generic mul=behz ks=bsplit_big");
    EQ(mul(with(f13, NO_FP64), 4), "generic mul=behz ks=lds_int guard=0 lazy=1");
    EQ(rot(with(f13, SW(no_galois_fusion)), 4), "permute bsplit_big");
    EQ(rot(with(f13, SW(no_split)), 4), "permute bsplit_big");  // NO_SPLIT stops the fold, not the sequence
    EQ(rot(with(f13, SW(no_fused)), 4), "permute bsplit_big");

    const RouteFacts f14 = facts(BFV, 14, {48, 48, 48, 49, 49, 49, 49, 49, 49});
    EQ(mul(f14, 8), "bmul");
    EQ(bmul(f14), "bmul");
    EQ(ks(f14, 8), "bsplit14 pass0=per_target");
    EQ(rot(f14, 8), "fold bsplit14 pass0=per_target");
    EQ(rot(f14, 8, 40), "fold bsplit14 pass0=per_limb");  // 20 ciphertexts per chunk, 160 pairs
    EQ(mul(with(f14, SW(no_bmul)), 8), "generic mul=behz ks=bsplit14 pass0=per_target");
    EQ(mul(with(f14, SW(no_bsplit)), 8), "generic mul=behz ks=lds_fp");
    EQ(bmul(with(f14, SW(no_bsplit))), "behz");
    EQ(rot(with(f14, SW(no_bsplit)), 8), "permute lds_fp");
    EQ(rot(with(f14, SW(no_galois_fusion)), 8), "permute bsplit14 pass0=per_target");
    EQ(mul(with(f14, SW(no_split)), 8), "generic mul=behz ks=lds_fp");
    EQ(mul(with(f14, SW(no_fused)), 8), "generic mul=behz ks=generic front=plain");
    EQ(mul(with(f14, BEHZ_INT), 8), "generic mul=behz ks=bsplit14 pass0=per_target");
    EQ(mul(with(f14, NO_FP64), 8), "generic mul=behz ks=lds_int guard=0 lazy=1");
    EQ(rot(with(f14, NO_FP64), 8), "permute lds_int guard=0 lazy=1");

    const RouteFacts f15 = facts(BFV, 15, chain(55, 55, 14, 56), false);
    EQ(mul(f15, 15), "generic mul=behz ks=generic front=iks guard=0");
    EQ(rot(f15, 15), "fold generic front=iks guard=0");
    EQ(rot(f15, 15, 1, true), "permute generic front=iks guard=0");
    EQ(rot(with(f15, SW(no_galois_fusion)), 15), "permute generic front=iks guard=0");
    EQ(rot(with(f15, SW(no_iks)), 15), "permute generic front=plain");
    EQ(bmul(f15), "behz");
  });

  t.run("config 5 (N = 2^16) and config 4 (N = 2^15)", [&] {
    const RouteFacts f16 = facts(BFV, 16, chain(55, 55, 7, 56), false);
    EQ(mul(f16, 8), "generic mul=behz ks=generic front=iks guard=0");
    EQ(rot(f16, 8), "fold generic front=iks guard=0");
    EQ(mul(with(f16, SW(no_iks)), 8), "generic mul=behz ks=generic front=plain");
    const RouteFacts g16 = facts(BFV, 16, chain(49, 49, 7, 50));  // the chain below 2^50
    EQ(mul(g16, 8), "generic mul=bmul_big ks=bsplit_big");
    EQ(rot(g16, 8), "fold bsplit_big");
    EQ(mul(with(g16, SW(no_gsplit)), 8), "generic mul=behz ks=generic front=fp");
    EQ(rot(with(g16, SW(no_gsplit)), 8), "permute generic front=fp");
    EQ(mul(with(g16, SW(no_bmul)), 8), "generic mul=behz ks=bsplit_big");
    EQ(mul(with(g16, NO_FP64), 8), "generic mul=behz ks=generic front=iks guard=0");

    const RouteFacts f = facts(CKKS, 15, {50, 40, 40, 50});
    EQ(mul(f, 3), "gsplit15");
    EQ(ks(f, 3), "gsplit15");
    EQ(rot(f, 3), "fold gsplit15");
    EQ(rot(f, 3, 1, true), "permute gsplit15");
    EQ(resc(f, 3), "generic");
    EQ(mul(with(f, SW(no_gsplit)), 3), "generic mul=tensor ks=generic front=fp");
    EQ(mul(with(f, SW(no_fused)), 3), "gsplit15");  // gsplit15 honours neither NO_FUSED nor NO_SPLIT ...
    EQ(mul(with(f, SW(no_split)), 3), "gsplit15");
    EQ(mul(with(f, NO_FP64), 3), "isplit15 guard=0 fpmask=0x0");
    const RouteFacts w = facts(CKKS, 15, {60, 40, 40, 60});
    EQ(mul(w, 3), "isplit15 guard=1 fpmask=0x6");
    EQ(rot(w, 3), "fold isplit15 guard=1 fpmask=0x6");
    EQ(mul(with(w, SW(no_fused)), 3), "generic mul=tensor ks=generic front=iks guard=1");  // ... isplit15 honours both
    EQ(mul(with(w, SW(no_split)), 3), "generic mul=tensor ks=generic front=iks guard=1");
    EQ(mul(with(w, SW(no_gsplit)), 3), "generic mul=tensor ks=generic front=iks guard=1");
    EQ(mul(with(w, SW(no_isplit)), 3), "generic mul=tensor ks=generic front=iks guard=1");
    EQ(mul(with(with(w, SW(no_isplit)), SW(no_iks)), 3), "generic mul=tensor ks=generic front=plain");
  });

  t.run("limb-count boundaries", [&] {
    const RouteFacts fp = facts(CKKS, 14, chain(50, 40, 13, 50));  // 14 data limbs below 2^50
    EQ(mul(fp, 5), "split14 front=lean pack=1 main=split4");
    EQ(mul(fp, 6), "split14 front=lean pack=0 main=split3");
    EQ(mul(fp, 12), "split14 front=lean pack=0 main=split3");
    EQ(mul(fp, 13), "lds_fp");
    EQ(ks(fp, 13), "lds_fp");
    EQ(rot(fp, 12), "fold split14 front=lean pack=0 main=split3");
    EQ(rot(fp, 12, 1, true), "permute split14 front=lean pack=0 main=split3");
    EQ(rot(fp, 13), "permute lds_fp");  // the LDS-resident kernels have no gather: k_galois first
    EQ(rot(fp, 13, 1, true), "permute lds_fp");
    const RouteFacts fp15 = facts(CKKS, 14, chain(50, 40, 14, 50));  // the deepest chain a context accepts
    EQ(rot(fp15, 12), "fold split14 front=lean pack=0 main=split3");
    EQ(rot(fp15, 15), "permute lds_fp");
    EQ(rot(fp15, 15, 3), "permute lds_fp");
    EQ(rot(fp15, 15, 1, true), "permute lds_fp");
    for (int nl = 1; nl <= 15; nl++) {  // a fold names a sequence that gathers, at every level and for every switch
      for (auto set : {+SW(no_split), +SW(no_fused), +SW(no_isplit), +SW(no_split4), +SW(no_lean_front), +SW(no_mixed), +SW(no_gsplit)})
        for (bool int_only : {false, true}) {
          RouteFacts g = with(fp15, set);
          if (int_only) g = with(g, NO_FP64);
          const RotRoute r = route_rotate(g, nl, false);
          EXPECT_TRUE(!r.fold || r.ks.seq == Seq::split14 || r.ks.seq == Seq::isplit);
        }
    }
    const RouteFacts wide = facts(CKKS, 14, chain(60, 40, 8, 60));
    EQ(mul(wide, 7), "isplit14 guard=1 fpmask=0x7e");
    EQ(mul(wide, 8), "lds_int guard=1 lazy=0");
    EQ(rot(wide, 7), "fold isplit14 guard=1 fpmask=0x7e");
    EQ(rot(wide, 8), "permute lds_int guard=1 lazy=0");
    EQ(ks(facts(BFV, 14, chain(48, 48, 7, 49)), 8), "bsplit14 pass0=per_target");
    EQ(ks(facts(BFV, 14, chain(48, 48, 8, 49)), 9), "lds_fp");
    EQ(ks(facts(BFV, 13, chain(48, 48, 7, 49)), 8), "bsplit_big");
    EQ(ks(facts(BFV, 13, chain(48, 48, 8, 49)), 9), "lds_fp");
    EQ(ks(facts(BFV, 16, chain(48, 48, 8, 49)), 9), "generic front=fp");
    EQ(mul(facts(CKKS, 15, chain(50, 40, 14, 50)), 15), "gsplit15");
    EQ(mul(facts(CKKS, 15, chain(50, 40, 15, 50)), 16), "generic mul=tensor ks=generic front=fp");
    EQ(mul(facts(CKKS, 15, chain(60, 40, 14, 60)), 15), "isplit15 guard=1 fpmask=0x7ffe");
    EQ(mul(facts(CKKS, 15, chain(60, 40, 15, 60)), 16), "generic mul=tensor ks=generic front=iks guard=1");
    EQ(mul(facts(CKKS, 13, HEAD), 4), "lds_fp");
    EQ(rot(facts(CKKS, 13, HEAD), 4), "permute lds_fp");
    EQ(mul(facts(CKKS, 16, HEAD), 4), "generic mul=tensor ks=generic front=fp");
  });

  t.run("per-chunk boundaries: lean limit, per-target limit, lanes, chunk caps", [&] {
    const RouteFacts f = facts(CKKS, 14, HEAD);
    EQ(mul(f, 4, 48), "split14 front=lean pack=1 main=split4");  // two lanes: 24 ciphertexts per chunk, 96 pairs
    EQ(mul(f, 4, 50), "split14 front=fat pack=1 main=split4");   // 25 per chunk
    const RouteFacts one = with(f, [](RouteFacts &g) { g.sw.lanes = 1; });
    EQ(mul(one, 4, 24), "split14 front=lean pack=1 main=split4");
    EQ(mul(one, 4, 25), "split14 front=fat pack=1 main=split4");
    EXPECT_TRUE(route_chunk(f, Seq::split14, 4, 24).lean);
    EXPECT_TRUE(!route_chunk(f, Seq::split14, 4, 25).lean);
    EQ(mul(with(f, [](RouteFacts &g) { g.sw.lean_limit = 3; }), 4), "split14 front=fat pack=1 main=split4");
    const RouteFacts b = facts(BFV, 14, chain(48, 48, 7, 49));
    EQ(ks(b, 8, 30), "bsplit14 pass0=per_target");  // 15 per chunk: 120 pairs, below 128
    EQ(ks(b, 8, 32), "bsplit14 pass0=per_limb");    // 16 per chunk: 128
    EXPECT_TRUE(route_chunk(b, Seq::bsplit14, 1, 127).per_target);
    EXPECT_TRUE(!route_chunk(b, Seq::bsplit14, 1, 128).per_target);
    ChunkPlan p = plan_chunks(f, 4, 8);
    EXPECT_TRUE(p.lanes == 1 && p.chunk == 8);
    p = plan_chunks(f, 4, 9);
    EXPECT_TRUE(p.lanes == 2 && p.chunk == 5);
    p = plan_chunks(f, 4, 256);
    EXPECT_TRUE(p.lanes == 2 && p.chunk == 128);
    p = plan_chunks(f, 4, 258);
    EXPECT_TRUE(p.lanes == 2 && p.chunk == 128);  // the cap: 129 would be an even split
    p = plan_chunks(f, 4, 8192);
    EXPECT_TRUE(p.chunk == 128);
    p = plan_chunks(facts(CKKS, 14, chain(50, 40, 13, 50)), 12, 1000);
    EXPECT_TRUE(p.chunk == 70);  // 4 GiB of scratch over two lanes at 232 limbs of 128 KiB per ciphertext
    p = plan_chunks(with(f, [](RouteFacts &g) { g.sw.chunk = 3; }), 4, 11);
    EXPECT_TRUE(p.chunk == 3 && p.lanes == 2);
    p = plan_chunks(with(f, [](RouteFacts &g) { g.sw.chunk = 300; }), 4, 11);
    EXPECT_TRUE(p.chunk == 11);
  });

  t.run("prime-width boundaries", [&] {
    EQ(mul(facts(CKKS, 14, {50, 40, 40, 50}), 3), "split14 front=lean pack=1 main=split4");
    EQ(mul(facts(CKKS, 14, {50, 40, 40, 51}), 3), "isplit14 guard=0 fpmask=0x7");
    EQ(mul(facts(CKKS, 14, {51, 40, 40, 50}), 3), "isplit14 guard=0 fpmask=0x6");
    EQ(resc(facts(CKKS, 14, {50, 40, 40, 51}), 3), "fp");  // the special prime is not in a rescale
    EQ(resc(facts(CKKS, 14, {51, 40, 40, 50}), 3), "mixed fpmask=0x6");
    EQ(ks(facts(CKKS, 16, {50, 40, 40, 50}), 3), "generic front=fp");
    EQ(ks(facts(CKKS, 16, {50, 40, 40, 51}), 3), "generic front=iks guard=0");
    EQ(ks(facts(CKKS, 16, {50, 40, 51, 50}), 2), "generic front=fp");  // the primes of the level, not of the chain
    const auto v1 = [](std::vector<int> b) { return with(facts(CKKS, 14, b), SW(no_isplit)); };
    EQ(mul(v1({55, 55, 55, 55}), 3), "lds_int guard=0 lazy=1");
    EQ(mul(v1({55, 55, 55, 56}), 3), "lds_int guard=0 lazy=0");
    EQ(mul(v1({57, 55, 55, 55}), 3), "lds_int guard=0 lazy=0");
    EQ(mul(v1({58, 55, 55, 55}), 3), "lds_int guard=1 lazy=0");
    EQ(mul(facts(CKKS, 14, {57, 40, 40, 57}), 3), "isplit14 guard=0 fpmask=0x6");
    EQ(mul(facts(CKKS, 14, {57, 40, 40, 58}), 3), "isplit14 guard=1 fpmask=0x6");
    EQ(mul(facts(CKKS, 14, {60, 40, 40, 60}), 3), "isplit14 guard=1 fpmask=0x6");
    EQ(mul(facts(CKKS, 14, {61, 40, 40, 60}), 3), "lds_int guard=1 lazy=0");
    EQ(mul(facts(CKKS, 15, {61, 40, 40, 60}), 3), "generic mul=tensor ks=generic front=iks guard=1");
    EQ(ks(facts(BFV, 14, chain(48, 48, 7, 50)), 8), "bsplit14 pass0=per_target");
    EQ(ks(facts(BFV, 14, chain(48, 48, 7, 51)), 8), "lds_int guard=0 lazy=1");
  });

  t.run("BFV big rings: the fold into the generic sequence is the integer fused front, and nothing else", [&] {
    const int W[] = {40, 49, 50, 51, 55, 57, 58, 60, 61};
    int folded = 0;
    for (int logn : {15, 16})
      for (int L : {1, 4, 8, 9, 15})
        for (int d : W)
          for (int s : W)
            for (int sw = 0; sw < 7; sw++) {
              RouteFacts f = facts(BFV, logn, chain(d, d, L - 1, s), d <= 50);
              if (sw == 1) f.sw.no_iks = true;
              if (sw == 2) f.sw.no_bsplit = true;
              if (sw == 3) f.sw.no_gsplit = true;
              if (sw == 4) f.use_fp = false;
              if (sw == 5) f.sw.no_fused = true;
              if (sw == 6) f.sw.no_split = true;
              f.finish();
              const RotRoute r = route_rotate(f, L, false);
              const KsRoute k = route_keyswitch(f, L);
              const bool fold_generic = r.fold && r.ks.seq == Seq::generic;
              EXPECT_TRUE(fold_generic == (k.seq == Seq::generic && k.front == KsFront::iks));
              if (fold_generic) {
                EXPECT_TRUE(r.ks.front == KsFront::iks);
                folded++;
              }
              EXPECT_TRUE(!route_rotate(with(f, SW(no_galois_fusion)), L, false).fold && !route_rotate(f, L, true).fold);
            }
    EXPECT_TRUE(folded > 0);
  });

  t.run("short buffer and unknown operation", [&] {
    char b[64];
    volatile size_t cap = 8;  // a caller's short buffer
    const RouteFacts f = facts(CKKS, 14, HEAD);
    EXPECT_TRUE(format_op(b, cap, f, kRouteMulRelin, 4, 1, false) == -1);
    EXPECT_TRUE(format_op(b, cap, f, kRouteMultiply, 4, 1, false) == 6 && std::string(b) == "tensor");
    EXPECT_TRUE(format_op(b, cap, f, 9, 4, 1, false) == -2);
  });
  return t.summary();
}
