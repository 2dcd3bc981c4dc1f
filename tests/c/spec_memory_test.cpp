// Drives the policy of dctz_spec_memory.h (the sf guess from the last verified statistics of the same input) on the CPU:
// streaks, what starts one again, the back-off after a wrong remembered guess, replacement of the least recently used
// entry, the clear.  Stand-alone: built with -fsanitize=address,undefined by tests/test_spec_memory_cpu.py.
#include <cstdio>
#include <cstdlib>
#include "dctz_spec_memory.h"

using dctz::SpecMemory;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main() {
  static double bufs[16][4];
  const int F64 = 1, F32 = 0;
  SpecMemory* m = new SpecMemory();       // (on the heap: an index past e[] is the sanitizer's to find)

  // ---- a streak: NEED_FIRST verified calls with one sf, then the entry predicts ----
  CHECK(m->predict(bufs[0], 100, F64) == nullptr);
  m->verified(bufs[0], 100, F64, 55.0, 0.001, 100.0);
  CHECK(m->predict(bufs[0], 100, F64) == nullptr);
  m->verified(bufs[0], 100, F64, 56.0, 0.002, 100.0);
  const SpecMemory::Entry* e = m->predict(bufs[0], 100, F64);
  CHECK(e != nullptr);
  if (e) CHECK(e->max_abs == 56.0 && e->min_abs == 0.002 && e->sf == 100.0 && e->streak == 2 && e->need == 2);
  // the key is all three of (address, length, element type)
  CHECK(m->predict(bufs[1], 100, F64) == nullptr);
  CHECK(m->predict(bufs[0], 101, F64) == nullptr);
  CHECK(m->predict(bufs[0], 100, F32) == nullptr);
  // a remembered guess that verifies keeps the streak going and refreshes the statistics
  m->verified(bufs[0], 100, F64, 57.0, 0.003, 100.0);
  e = m->predict(bufs[0], 100, F64);
  CHECK(e && e->streak == 3 && e->max_abs == 57.0);

  // ---- another verified sf (a sampled call saw the decade change): the streak starts again, need stays ----
  m->verified(bufs[0], 100, F64, 570.0, 0.003, 1000.0);
  CHECK(m->predict(bufs[0], 100, F64) == nullptr);
  m->verified(bufs[0], 100, F64, 571.0, 0.003, 1000.0);
  e = m->predict(bufs[0], 100, F64);
  CHECK(e && e->sf == 1000.0 && e->streak == 2 && e->need == 2);

  // ---- a wrong remembered guess: streak 0, need doubled, up to NEED_MAX ----
  unsigned want = 2;
  for (int round = 0; round < 8; round++) {
    m->missed(bufs[0], 100, F64, true);
    want = want * 2 < SpecMemory::NEED_MAX ? want * 2 : SpecMemory::NEED_MAX;
    CHECK(m->find(bufs[0], 100, F64) && m->find(bufs[0], 100, F64)->need == want && m->find(bufs[0], 100, F64)->streak == 0);
    for (unsigned i = 0; i < want; i++) {
      CHECK(m->predict(bufs[0], 100, F64) == nullptr);
      m->verified(bufs[0], 100, F64, 5.0, 0.5, 10.0);
    }
    CHECK(m->predict(bufs[0], 100, F64) != nullptr);
  }
  CHECK(want == 64 && SpecMemory::NEED_MAX == 64);
  // a wrong SAMPLED guess ends the streak and leaves need alone; on an unknown key it does nothing
  m->missed(bufs[0], 100, F64, false);
  CHECK(m->find(bufs[0], 100, F64)->need == 64 && m->find(bufs[0], 100, F64)->streak == 0);
  m->missed(bufs[9], 100, F64, true);
  CHECK(m->find(bufs[9], 100, F64) == nullptr);

  // ---- replacement: SLOTS keys fit, one more replaces the least recently touched ----
  m->clear();
  for (int k = 0; k < SpecMemory::SLOTS; k++) {
    m->verified(bufs[k], 64, F32, 1.0 + k, 0.5, 10.0);
    m->verified(bufs[k], 64, F32, 1.0 + k, 0.5, 10.0);
  }
  for (int k = 0; k < SpecMemory::SLOTS; k++) CHECK(m->predict(bufs[k], 64, F32) != nullptr);
  CHECK(m->predict(bufs[0], 64, F32) != nullptr);           // key 0 is now the most recently touched, key 1 the least
  m->verified(bufs[8], 64, F32, 9.0, 0.5, 10.0);
  CHECK(m->find(bufs[1], 64, F32) == nullptr);
  CHECK(m->find(bufs[8], 64, F32) != nullptr && m->find(bufs[8], 64, F32)->streak == 1 && m->find(bufs[8], 64, F32)->need == 2);
  for (int k = 0; k < SpecMemory::SLOTS; k++) if (k != 1) CHECK(m->find(bufs[k], 64, F32) != nullptr);
  // many more keys than slots: always SLOTS live entries, the newest present
  for (int round = 0; round < 5; round++)
    for (int k = 0; k < 16; k++) {
      m->verified(bufs[k], 64, F32, 1.0, 0.5, 10.0);
      CHECK(m->find(bufs[k], 64, F32) != nullptr);
      int live = 0;
      for (const SpecMemory::Entry& x : m->e) live += x.stamp != 0;
      CHECK(live == SpecMemory::SLOTS);
    }

  // ---- the clear ----
  m->clear();
  for (int k = 0; k < 16; k++) CHECK(m->find(bufs[k], 64, F32) == nullptr && m->predict(bufs[k], 64, F32) == nullptr);
  m->verified(bufs[3], 64, F32, 1.0, 0.5, 10.0);
  CHECK(m->find(bufs[3], 64, F32)->need == SpecMemory::NEED_FIRST && m->find(bufs[3], 64, F32)->streak == 1);

  delete m;
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("spec memory ok\n");
  return 0;
}
