// The owner table of abc_hip_malloc blocks and context buffers (abc_amd/csrc/abc_buffers.hpp) on made-up pointers: no GPU, no
// driver.  Every case checks the table's answers, the cached-bytes figure and the count of held-back context buffers.
#include <algorithm>

#include "../../abc_amd/csrc/abc_buffers.hpp"
#include "mini_test.hpp"

using abc::BufferTable;
using Take = BufferTable::Take;
using Release = BufferTable::Release;

static void *P(uintptr_t i) { return (void *)(i << 12); }
static void *const G1 = (void *)(uintptr_t)0xa000001, *const G2 = (void *)(uintptr_t)0xa000002;
static const std::vector<void *> kNone;

static std::vector<void *> sorted(std::vector<void *> v) {
  std::sort(v.begin(), v.end());
  return v;
}
// what abc_hip_malloc does outside the table: a miss goes to the driver (here: pointer `fresh`) and is registered
static void *alloc(BufferTable &t, size_t size, void *fresh) {
  void *p = nullptr;
  const Take r = t.take(size, &p);
  if (r == Take::hit) return p;
  if (r == Take::refused) return nullptr;
  t.add_block(fresh, size);
  return fresh;
}
#define EXPECT_STATE(t, bytes, held_count) EXPECT_TRUE((t).cached_bytes() == (size_t)(bytes) && (t).held() == (size_t)(held_count))

int main() {
  MiniTest mt;

  mt.run("1 exact-size cache, cap, trim", [] {
    BufferTable t;
    t.cache_cap = 300;
    void *p = nullptr;
    EXPECT_TRUE(t.take(100, &p) == Take::miss);
    t.add_block(P(1), 100);
    EXPECT_TRUE(t.release(P(1)) == Release::cached);
    EXPECT_STATE(t, 100, 0);
    EXPECT_TRUE(t.take(104, &p) == Take::miss);  // a different size misses
    EXPECT_TRUE(t.take(100, &p) == Take::hit && p == P(1));
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.release(P(1)) == Release::cached);
    t.add_block(P(2), 200);
    EXPECT_TRUE(t.release(P(2)) == Release::cached);  // exactly at the cap
    EXPECT_STATE(t, 300, 0);
    t.add_block(P(3), 8);
    EXPECT_TRUE(t.release(P(3)) == Release::over_cap);  // the caller trims and frees P(3) itself
    EXPECT_TRUE(sorted(t.trim()) == sorted({P(1), P(2)}));
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.trim() == kNone);
    EXPECT_TRUE(t.take(100, &p) == Take::miss);
    EXPECT_TRUE(t.release(P(9)) == Release::untracked);  // never registered (cache switched off): freed by the caller
    EXPECT_TRUE(t.drain() == kNone);                      // trim and over_cap forgot their blocks
  });

  mt.run("2 block taken from the cache and freed inside a capture", [] {
    BufferTable t;
    t.add_block(P(1), 64);
    EXPECT_TRUE(t.release(P(1)) == Release::cached);
    t.begin_capture();
    void *p = nullptr;
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.release(P(1)) == Release::parked);
    EXPECT_STATE(t, 0, 0);  // not in the cache: reusable inside this capture only
    p = nullptr;
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));  // handed out again inside the same capture
    EXPECT_TRUE(t.release(P(1)) == Release::parked);
    EXPECT_TRUE(t.end_capture(G1) == kNone);
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.take(64, &p) == Take::miss);  // parked, not cached
    EXPECT_TRUE(t.drop_owner(G1) == kNone);
    EXPECT_STATE(t, 64, 0);
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));
  });

  mt.run("3 block out with the caller at the end of a capture, freed later", [] {
    BufferTable t;
    t.add_block(P(1), 64);
    t.begin_capture();
    EXPECT_TRUE(t.end_capture(G1) == kNone);
    EXPECT_TRUE(t.release(P(1)) == Release::parked);
    EXPECT_STATE(t, 0, 0);
    void *p = nullptr;
    EXPECT_TRUE(t.take(64, &p) == Take::miss);
    EXPECT_TRUE(t.drop_owner(G1) == kNone);
    EXPECT_STATE(t, 64, 0);
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));
    EXPECT_TRUE(t.release(P(1)) == Release::cached);  // no graph left: an ordinary block again
  });

  mt.run("4 block from before the capture, freed inside it", [] {
    BufferTable t;
    t.add_block(P(1), 64);
    t.add_block(P(2), 64);
    EXPECT_TRUE(t.release(P(2)) == Release::cached);
    t.begin_capture();
    EXPECT_TRUE(t.release(P(1)) == Release::parked);  // an input of every replay
    void *p = nullptr;
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(2));  // the cached block, never the parked one
    EXPECT_TRUE(t.take(64, &p) == Take::refused);
    EXPECT_TRUE(t.end_capture(G1) == kNone);
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.take(64, &p) == Take::miss);
    EXPECT_TRUE(t.drop_owner(G1) == kNone);
    EXPECT_STATE(t, 64, 0);  // P(1) is back; P(2) is still out with the caller
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));
  });

  mt.run("5 two graphs own one block", [] {
    BufferTable t;
    t.add_block(P(1), 64);
    t.begin_capture();
    EXPECT_TRUE(t.end_capture(G1) == kNone);
    t.begin_capture();
    EXPECT_TRUE(t.end_capture(G2) == kNone);
    EXPECT_TRUE(t.release(P(1)) == Release::parked);
    EXPECT_TRUE(t.drop_owner(G1) == kNone);
    EXPECT_STATE(t, 0, 0);  // still parked for the second graph
    void *p = nullptr;
    EXPECT_TRUE(t.take(64, &p) == Take::miss);
    EXPECT_TRUE(t.drop_owner(G2) == kNone);
    EXPECT_STATE(t, 64, 0);
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));
  });

  mt.run("6 abandoned capture", [] {
    BufferTable t;
    t.add_block(P(1), 64);  // freed inside: pinned as an input
    t.add_block(P(2), 32);  // born and freed inside
    t.add_block(P(3), 16);  // born inside, still out at the end
    EXPECT_TRUE(t.release(P(2)) == Release::cached);
    EXPECT_TRUE(t.release(P(3)) == Release::cached);
    EXPECT_STATE(t, 48, 0);
    t.begin_capture();
    void *p = nullptr;
    EXPECT_TRUE(t.release(P(1)) == Release::parked);
    EXPECT_TRUE(t.take(32, &p) == Take::hit && p == P(2));
    EXPECT_TRUE(t.release(P(2)) == Release::parked);
    EXPECT_TRUE(t.take(16, &p) == Take::hit && p == P(3));
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.end_capture(nullptr) == kNone);
    EXPECT_TRUE(!t.capturing);
    EXPECT_STATE(t, 64 + 32, 0);  // nothing stays pinned: both freed blocks are ordinary cached blocks again
    EXPECT_TRUE(t.take(64, &p) == Take::hit && p == P(1));
    EXPECT_TRUE(t.take(32, &p) == Take::hit && p == P(2));
    EXPECT_TRUE(t.release(P(3)) == Release::cached);  // no owner left behind on the block that was out
  });

  mt.run("7 a capture never reaches the driver", [] {
    BufferTable t;
    t.begin_capture();
    EXPECT_TRUE(alloc(t, 64, P(1)) == nullptr);
    void *p = nullptr;
    EXPECT_TRUE(t.take(64, &p) == Take::refused);
    EXPECT_TRUE(t.end_capture(nullptr) == kNone);
    EXPECT_TRUE(t.take(64, &p) == Take::miss);  // outside: a miss, the caller allocates
    EXPECT_STATE(t, 0, 0);
  });

  mt.run("8 context buffer alive at the end of a graph / registered after it", [] {
    BufferTable t;
    t.add_context_buffer(P(1), 1000);
    t.begin_capture();
    EXPECT_TRUE(t.end_capture(G1) == kNone);
    t.add_context_buffer(P(2), 2000);  // a key or mirror made after the recording: the graph cannot know it
    EXPECT_TRUE(!t.retire(P(1)));
    EXPECT_STATE(t, 0, 1);
    EXPECT_TRUE(t.retire(P(2)));  // freed at once
    EXPECT_STATE(t, 0, 1);
    EXPECT_TRUE(t.drop_owner(G1) == std::vector<void *>{P(1)});
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.drain() == kNone);  // a context buffer never enters the cache
    t.add_context_buffer(P(3), 8);
    EXPECT_TRUE(t.retire(P(3)));  // no graph at all
  });

  for (int newer_first = 0; newer_first < 2; newer_first++)
    mt.run(newer_first ? "9 two graphs, growth in between, newer destroyed first" : "9 two graphs, growth in between, older destroyed first",
           [newer_first] {
             BufferTable t;
             t.add_context_buffer(P(1), 100);  // workspace of graph 1
             t.add_context_buffer(P(7), 50);   // a key both graphs read
             t.begin_capture();
             EXPECT_TRUE(t.end_capture(G1) == kNone);
             EXPECT_TRUE(!t.retire(P(1)));  // graph 2's eager pass grows the workspace
             t.add_context_buffer(P(2), 200);
             EXPECT_STATE(t, 0, 1);
             t.begin_capture();
             EXPECT_TRUE(t.end_capture(G2) == kNone);
             EXPECT_TRUE(!t.retire(P(2)));  // growth after both
             t.add_context_buffer(P(3), 400);
             EXPECT_STATE(t, 0, 2);  // one workspace per graph: P(2) was allocated after graph 1 had ended
             if (newer_first) {
               EXPECT_TRUE(t.drop_owner(G2) == std::vector<void *>{P(2)});
               EXPECT_STATE(t, 0, 1);
               EXPECT_TRUE(t.drop_owner(G1) == std::vector<void *>{P(1)});
             } else {
               EXPECT_TRUE(t.drop_owner(G1) == std::vector<void *>{P(1)});
               EXPECT_STATE(t, 0, 1);
               EXPECT_TRUE(t.drop_owner(G2) == std::vector<void *>{P(2)});
             }
             EXPECT_STATE(t, 0, 0);
             EXPECT_TRUE(t.retire(P(7)) && t.retire(P(3)));  // nobody owns them any more
           });

  mt.run("10 final enumeration", [] {
    BufferTable t;
    t.add_block(P(1), 64);            // cached
    t.add_block(P(2), 64);            // parked
    t.add_block(P(3), 64);            // out with the caller
    t.add_context_buffer(P(4), 100);  // held back
    t.add_context_buffer(P(5), 100);  // in use
    EXPECT_TRUE(t.release(P(1)) == Release::cached);
    t.begin_capture();
    EXPECT_TRUE(t.end_capture(G1) == kNone);
    EXPECT_TRUE(t.release(P(2)) == Release::parked);
    EXPECT_TRUE(!t.retire(P(4)));
    EXPECT_STATE(t, 64, 1);
    EXPECT_TRUE(sorted(t.drain()) == sorted({P(1), P(2), P(3), P(4), P(5)}));
    EXPECT_STATE(t, 0, 0);
    EXPECT_TRUE(t.drain() == kNone);
    EXPECT_TRUE(t.drop_owner(G1) == kNone);
  });

  return mt.summary();
}
