// Speculation on the last VERIFIED statistics of the same input (host only: plain C++, no HIP).
//
// A speculative compress call guesses the decade of max|x| -- that is all the scaling factor depends on (util.c:29) --
// lets k_compress compute the true statistics on the way, and verifies the guess afterwards.  The guess comes from a
// 1/64 sample (two launches in front of k_compress) or, for a caller that compresses the same buffer call after call,
// from this table: the true statistics of the last call on (address, length, element type) whose guess verified.
// Such a guess costs no launch.  The table only PREDICTS; the check behind the pass does not depend on it.
//
// Policy:
//   - a key is used once `streak` consecutive verified speculative calls on it chose the same scaling factor,
//     streak >= need; need starts at NEED_FIRST;
//   - a verified call with another scaling factor starts the streak again (need stays);
//   - a guess from the table that the true statistics refuse sets streak = 0 and doubles need (at most NEED_MAX): a caller
//     that rotates unrelated fields through one buffer loses a bounded share of its calls to re-runs;
//   - SLOTS entries, the least recently touched one replaced.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dctz {

struct SpecMemory {
  static constexpr int SLOTS = 8;
  static constexpr unsigned NEED_FIRST = 2, NEED_MAX = 64;
  struct Entry {
    const void* ptr = nullptr;
    size_t n = 0;
    int dtype = -1;
    double max_abs = 0.0, min_abs = 0.0;   // true statistics of the last verified call on this key
    double sf = 0.0;                       // ... and its scaling factor
    unsigned streak = 0, need = NEED_FIRST;
    unsigned long long stamp = 0;          // 0: free
  };
  Entry e[SLOTS];
  unsigned long long clock = 0;

  void clear() { for (Entry& x : e) x = Entry(); clock = 0; }

  Entry* find(const void* ptr, size_t n, int dtype) {
    for (Entry& x : e) if (x.stamp && x.ptr == ptr && x.n == n && x.dtype == dtype) return &x;
    return nullptr;
  }
  // The entry to guess from, or NULL: the key is unknown or its streak is too short.
  const Entry* predict(const void* ptr, size_t n, int dtype) {
    Entry* x = find(ptr, n, dtype);
    if (!x || x->streak < x->need) return nullptr;
    x->stamp = ++clock;
    return x;
  }
  // A speculative call on the key verified (whichever the source of its guess): its true statistics and scaling factor.
  void verified(const void* ptr, size_t n, int dtype, double max_abs, double min_abs, double sf) {
    Entry* x = find(ptr, n, dtype);
    if (!x) {
      x = &e[0];
      for (Entry& y : e) if (y.stamp < x->stamp) x = &y;      // a free slot (stamp 0), else the least recently touched
      *x = Entry();
      x->ptr = ptr; x->n = n; x->dtype = dtype;
    }
    if (x->streak && x->sf == sf) x->streak++;
    else x->streak = 1;
    x->max_abs = max_abs; x->min_abs = min_abs; x->sf = sf;
    x->stamp = ++clock;
  }
  // A speculative call on the key missed.  from_memory: the guess was this table's (else the sample's).
  void missed(const void* ptr, size_t n, int dtype, bool from_memory) {
    Entry* x = find(ptr, n, dtype);
    if (!x) return;
    x->streak = 0;
    if (from_memory) x->need = x->need * 2 < NEED_MAX ? x->need * 2 : NEED_MAX;
    x->stamp = ++clock;
  }
};

}  // namespace dctz
