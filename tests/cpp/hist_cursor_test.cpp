// CPU test of bourse_amd/csrc/hist_cursor.hpp (tests/test_hist_tables_cpu.py compiles and runs it): what a table folded from
// the level-2 history ring owes, as a function of its cursor, the env's step counter, the ring's base and its capacity.
// Cases worked out by hand first, then a ring that is really written: step s goes to slot s % cap, a cursor that folds at
// random moments must find step seen + i in slot_of(slot0, i, cap) for every i < n, and is told "lost" exactly when a step
// it has not folded was overwritten or cleared.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/hist_cursor.hpp"

using namespace bkd::ring;

static int failures = 0, cases = 0;

static void expect(const char* what, uint64_t seen, uint64_t done, uint64_t base, uint64_t cap, CursorKind kind, uint64_t first,
                   uint32_t slot0, uint32_t n) {
  const Cursor c = cursor(seen, done, base, cap);
  ++cases;
  const bool ok = c.kind == kind && c.first == first && (kind != CURSOR_FOLD || (c.slot0 == slot0 && c.n == n));
  if (ok) return;
  ++failures;
  std::printf("%s: cursor(%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 ") = {%d, %" PRIu64 ", %u, %u}, expected {%d, %" PRIu64
              ", %u, %u}\n",
              what, seen, done, base, cap, static_cast<int>(c.kind), c.first, c.slot0, c.n, static_cast<int>(kind), first, slot0, n);
}

// a ring of `cap` slots stepped `steps` times; the cursor folds when `fold_at(step)` says so, the ring is cleared at `clear_at`
static void walk(const char* what, uint64_t start, uint64_t cap, uint64_t steps, uint64_t fold_every, uint64_t clear_at) {
  std::vector<uint64_t> slot_step(cap, ~0ull);
  uint64_t done = start, base = start, seen = start;
  for (uint64_t q = 0; q < steps; ++q) {
    slot_step[done % cap] = done;
    ++done;
    if (q == clear_at) base = done;
    if ((q + 1) % fold_every) continue;
    ++cases;
    const Cursor c = cursor(seen, done, base, cap);
    // the truth: every step of [seen, done) is retained if it is >= base and still stands in its slot
    bool retained = true;
    for (uint64_t s = seen; s < done && retained; ++s) retained = s >= base && slot_step[s % cap] == s;
    bool ok = true;
    if (!retained) {
      ok = c.kind == CURSOR_LOST && c.first > seen && c.first <= done;
      // [seen, first) is exactly what is gone: step first (if any) is retained, step first - 1 is not
      if (ok && c.first < done) ok = c.first >= base && slot_step[c.first % cap] == c.first;
      if (ok) ok = c.first - 1 < base || slot_step[(c.first - 1) % cap] != c.first - 1;
      seen = done;  // (a full clear starts again)
    } else if (seen == done) {
      ok = c.kind == CURSOR_NOTHING;
    } else {
      ok = c.kind == CURSOR_FOLD && c.n == done - seen && c.n >= 1 && c.n <= cap && c.slot0 < cap;
      for (uint32_t i = 0; ok && i < c.n; ++i) ok = slot_step[slot_of(c.slot0, i, cap)] == seen + i;
      seen = done;
    }
    if (!ok) {
      ++failures;
      std::printf("%s: cap %" PRIu64 " step %" PRIu64 ": {%d, %" PRIu64 ", %u, %u}\n", what, cap, done, static_cast<int>(c.kind), c.first,
                  c.slot0, c.n);
      return;
    }
  }
}

int main() {
  const uint64_t G = 1ull << 32;
  expect("seen == done", 7, 7, 0, 8, CURSOR_NOTHING, 0, 0, 0);
  expect("seen == done, nothing stepped", 0, 0, 0, 8, CURSOR_NOTHING, 0, 0, 0);
  expect("seen == done == base", 9, 9, 9, 8, CURSOR_NOTHING, 9, 0, 0);
  expect("a ring of 1, one step", 4, 5, 0, 1, CURSOR_FOLD, 4, 0, 1);
  expect("a ring of 1, two steps", 3, 5, 0, 1, CURSOR_LOST, 4, 0, 0);
  expect("a ring of 1, up to date", 5, 5, 0, 1, CURSOR_NOTHING, 4, 0, 0);
  expect("done - seen == cap", 12, 20, 0, 8, CURSOR_FOLD, 12, 4, 8);
  expect("done - seen == cap + 1", 11, 20, 0, 8, CURSOR_LOST, 12, 0, 0);
  expect("base above done - cap, seen below it", 14, 20, 17, 8, CURSOR_LOST, 17, 0, 0);
  expect("base above done - cap, seen at it", 17, 20, 17, 8, CURSOR_FOLD, 17, 1, 3);
  expect("base == done, seen below", 19, 20, 20, 8, CURSOR_LOST, 20, 0, 0);
  expect("seen == first", 12, 19, 0, 7, CURSOR_FOLD, 12, 5, 7);
  expect("fewer steps than the ring", 0, 5, 0, 16, CURSOR_FOLD, 0, 0, 5);
  // above 2^32 with a capacity that does not divide 2^32: the slot is the 64-bit remainder, not the low word's
  expect("above 2^32", G + 5, G + 9, 0, 12, CURSOR_FOLD, G - 3, static_cast<uint32_t>((G + 5) % 12), 4);
  expect("above 2^32, cap 1000", 3 * G + 17, 3 * G + 1017, 0, 1000, CURSOR_FOLD, 3 * G + 17, static_cast<uint32_t>((3 * G + 17) % 1000), 1000);
  expect("above 2^32, lost", G + 5, G + 18, 0, 12, CURSOR_LOST, G + 6, 0, 0);
  expect("across 2^32", G - 2, G + 3, 0, 7, CURSOR_FOLD, G - 4, static_cast<uint32_t>((G - 2) % 7), 5);
  if ((G + 5) % 12 == static_cast<uint32_t>(G + 5) % 12u) ++failures, std::printf("the 2^32 case does not tell the remainders apart\n");
  // the largest ring: n and the slot still fit a u32
  expect("a ring of 2^32 - 1", G + 1, 2 * G, 0, G - 1, CURSOR_FOLD, G + 1, 2, 0xFFFFFFFFu);
  // the slot wraps inside one fold: slots 6, 7, 0, 1
  expect("the slot wraps", 14, 18, 0, 8, CURSOR_FOLD, 10, 6, 4);
  ++cases;
  if (slot_of(6, 0, 8) != 6 || slot_of(6, 1, 8) != 7 || slot_of(6, 2, 8) != 0 || slot_of(6, 3, 8) != 1 || slot_of(0, 0, 1) != 0 ||
      slot_of(0xFFFFFFFEu, 0xFFFFFFFEu, 0xFFFFFFFFull) != 0xFFFFFFFDull)
    ++failures, std::printf("slot_of\n");

  for (uint64_t cap : {1ull, 2ull, 3ull, 7ull, 8ull, 12ull})
    for (uint64_t every : {1ull, 2ull, 5ull, 7ull, 8ull, 9ull, 13ull}) {
      walk("walk", 0, cap, 100, every, ~0ull);
      walk("walk, cleared", 0, cap, 100, every, 40);
      walk("walk above 2^32", G - 30, cap, 100, every, 57);
    }

  if (failures) {
    std::printf("hist_cursor FAILED %d of %d\n", failures, cases);
    return 1;
  }
  std::printf("hist_cursor ok %d cases\n", cases);
  return 0;
}
