// abc_buffers.hpp -- the owner table of every device buffer a recorded circuit (abc_hip_graph_*) may read.  Plain C++: it never
// calls the driver; an operation that ends a buffer's life returns the pointers its caller must hipFree (abc_buffers.hip is that
// caller; tests/cpp/test_buffer_table.cpp drives the table with made-up pointers).  Its user serialises every call (alloc_mu).
//
// A graph bakes raw device pointers into its kernel arguments, so a buffer it may have recorded must outlive it.  ONE RULE: every
// buffer that is tracked, not yet released by its user and not in the cache when end_capture(owner) runs is owned by that graph
// until drop_owner(owner) -- a superset of what the sequence read, found without tracing a single kernel argument.  (A buffer
// released earlier cannot be in the recording, unless it was released DURING the capture: that is the sentinel owner below.)
// A buffer is either a CALLER BLOCK (abc_hip_malloc / abc_hip_free; recycled through an exact-size cache) or a CONTEXT BUFFER
// (workspace, arenas, keys, key mirrors; never recycled).  Released while owned, either kind stays where it is -- a caller block
// "parked", a context buffer "held back" -- and only what happens when its last owner goes differs: the block returns to the
// cache, the context buffer is handed back for hipFree.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace abc {

class BufferTable {
 public:
  enum class Take { hit, miss, refused };  // refused: a capture found no cached block (hipMalloc is not capturable)
  // cached / parked: nothing to do.  untracked: not in the table (the caller drains the stream and frees it).  over_cap: the same,
  // after freeing everything trim() returns: exact-size buckets strand blocks when sizes vary, so the whole cache goes
  enum class Release { cached, parked, untracked, over_cap };

  size_t cache_cap = (size_t)8 << 30;
  bool capturing = false;  // between begin_capture and end_capture

  size_t cached_bytes() const { return cached_bytes_; }
  // context buffers retired while owned (abc_hip_ctx_info 6); parked caller blocks are not counted
  size_t held() const {
    size_t n = 0;
    for (auto &kv : entries_) n += kv.second.context && kv.second.released;
    return n;
  }

  void add_block(void *p, size_t size) { entries_[p] = Entry{size, false, false, false, {}}; }
  void add_context_buffer(void *p, size_t size) { entries_[p] = Entry{size, true, false, false, {}}; }

  // A cached block of exactly `size`.  Inside a capture: a block born and freed in this capture first (safe: stream order inside
  // the graph), then the cache, never the driver -- the sequence must have run once eagerly before.
  Take take(size_t size, void **out) {
    if (capturing && pop(cap_free_, size, out)) return Take::hit;
    if (pop(free_blocks_, size, out)) {
      cached_bytes_ -= size;
      if (capturing) {
        Entry &e = entries_[*out];
        e.owners.push_back(kCapturing);
        e.cap_born = true;
      }
      return Take::hit;
    }
    return capturing ? Take::refused : Take::miss;
  }

  Release release(void *p) {
    auto it = entries_.find(p);
    if (it == entries_.end() || it->second.context) return Release::untracked;
    Entry &e = it->second;
    if (capturing) {
      if (e.cap_born) {  // an intermediate of the circuit being recorded: reusable inside it
        cap_free_[e.size].push_back(p);
        return Release::parked;
      }
      add_owner(e, kCapturing);  // existed before: the graph reads it as an input on every replay -- never reused
    }
    if (!e.owners.empty()) {
      e.released = true;
      return Release::parked;
    }
    if (cached_bytes_ + e.size <= cache_cap) {
      to_cache(p, e);
      return Release::cached;
    }
    entries_.erase(it);
    return Release::over_cap;
  }

  // a context buffer goes: true = free it now, false = held back for the graphs that own it
  bool retire(void *p) {
    auto it = entries_.find(p);
    if (it == entries_.end()) return true;
    if (!it->second.owners.empty()) {
      it->second.released = true;
      return false;
    }
    entries_.erase(it);
    return true;
  }

  void begin_capture() { capturing = true; }
  // owner = the recorded graph; nullptr = the capture was abandoned, what it had pinned is let go.  Returns what to free.
  std::vector<void *> end_capture(void *owner) {
    capturing = false;
    for (auto &kv : cap_free_)
      for (void *p : kv.second) entries_[p].released = true;  // born and freed inside the capture: nobody holds them any more
    cap_free_.clear();
    std::unordered_set<void *> cached;
    for (auto &kv : free_blocks_) cached.insert(kv.second.begin(), kv.second.end());
    for (auto &kv : entries_) {
      Entry &e = kv.second;
      e.cap_born = false;
      // the one rule, and what was released during the capture itself
      if (owner && ((!e.released && !cached.count(kv.first)) || has_owner(e, kCapturing))) add_owner(e, owner);
    }
    return drop_owner(kCapturing);
  }

  // a released buffer nobody owns any more: a caller block returns to the cache, a context buffer is returned for freeing
  std::vector<void *> drop_owner(void *owner) {
    std::vector<void *> to_free;
    for (auto it = entries_.begin(); it != entries_.end();) {
      Entry &e = it->second;
      const auto mine = std::find(e.owners.begin(), e.owners.end(), owner);
      const bool last = mine != e.owners.end() && e.owners.size() == 1;
      if (mine != e.owners.end()) e.owners.erase(mine);
      if (last && e.released) {
        if (e.context) {
          to_free.push_back(it->first);
          it = entries_.erase(it);
          continue;
        }
        e.released = false;
        to_cache(it->first, e);
      }
      ++it;
    }
    return to_free;
  }

  // every cached block, forgotten by the table
  std::vector<void *> trim() {
    std::vector<void *> out;
    for (auto &kv : free_blocks_)
      for (void *p : kv.second) {
        entries_.erase(p);
        out.push_back(p);
      }
    free_blocks_.clear();
    cached_bytes_ = 0;
    return out;
  }

  // every pointer still tracked -- cached, parked, held back, or out with its user -- once; the table is empty afterwards
  std::vector<void *> drain() {
    std::vector<void *> out;
    for (auto &kv : entries_) out.push_back(kv.first);
    entries_.clear();
    free_blocks_.clear();
    cap_free_.clear();
    cached_bytes_ = 0;
    return out;
  }

 private:
  struct Entry {
    size_t size;
    bool context;   // context buffer (else: caller block)
    bool released;  // its user is done with it; it stays for its owners
    bool cap_born;  // caller block taken from the cache during the running capture
    std::vector<void *> owners;  // graph handles, kCapturing for the capture in progress
  };
  using Buckets = std::unordered_map<size_t, std::vector<void *>>;
  static inline void *const kCapturing = (void *)(uintptr_t)1;

  static bool pop(Buckets &b, size_t size, void **out) {
    auto it = b.find(size);
    if (it == b.end() || it->second.empty()) return false;
    *out = it->second.back();
    it->second.pop_back();
    return true;
  }
  static bool has_owner(const Entry &e, void *owner) { return std::find(e.owners.begin(), e.owners.end(), owner) != e.owners.end(); }
  static void add_owner(Entry &e, void *owner) {
    if (!has_owner(e, owner)) e.owners.push_back(owner);
  }
  void to_cache(void *p, const Entry &e) {
    free_blocks_[e.size].push_back(p);
    cached_bytes_ += e.size;
  }

  std::unordered_map<void *, Entry> entries_;  // every tracked pointer
  Buckets free_blocks_;                         // size -> cached blocks
  Buckets cap_free_;                            // blocks born AND freed during the running capture, reusable inside it
  size_t cached_bytes_ = 0;
};

}  // namespace abc
