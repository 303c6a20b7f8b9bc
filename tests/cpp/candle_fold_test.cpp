// CPU test of bourse_amd/csrc/candle_fold.hpp (tests/test_candles_cpu.py compiles and runs it): the bar and slot of a step,
// which bars a fold skips, when a slot's row is continued, what one level-2 record adds to its bar, the merge of two parts
// and which lanes of the device fold form a bar's segment, over the series of <records file>, compared word for word with
// the rows and carry of <expected file>, which tests/candles_model.py printed.
//   records:  n_series, then per series one line "n_steps W N first_step n_folds" and n_folds pairs "end cut" (0 < end_1 < ..
//             = n_steps: the series is folded as [0, end_1), [end_1, end_2), ..; cut 1: the carry is zeroed in front of that
//             fold, as a reset does) and one line per step: trade_vol bid ask.  Step i of the series is absolute step
//             first_step + i.
//   expected: per series and fold N lines of 16 words and one line with the carry word after it
// Every fold is done twice.  "lanes": as the device kernel does it - passes of 64 lanes, a lane a step, the word of the step
// before from the lane below (lane 0: the pass before, or the carry), a head-flagged segmented scan in six rounds (each
// round reads the round before of the lane `off` below), every tail lane of a bar the fold does not skip loads its slot's
// row, and then they store, the highest lane first: no two may write one slot.  "serial": step by step into the slot of the
// step's bar, nothing skipped.  Both must give the expected rows and carry.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/candle_fold.hpp"

using namespace bkd::candles;

struct Rec {
  uint32_t tv, bid, ask;
};

struct Table {
  uint32_t W, N;
  std::vector<Part> rows;  // [N]
  uint64_t carry = 0ull;
  Table(uint32_t width, uint32_t n) : W(width), N(n), rows(n, cleared()) {}
};

// steps r[lo .. hi) are absolute steps first + lo .. first + hi
static int fold_lanes(Table& t, const std::vector<Rec>& r, uint64_t first, size_t lo, size_t hi) {
  const uint32_t n = static_cast<uint32_t>(hi - lo), W = t.W, N = t.N;
  const uint64_t seen = first + lo;
  Pass at = first_pass(seen, W, N);
  const uint64_t last_bar = bar_of(seen + n - 1u, W);
  uint64_t tail = t.carry, cur[64] = {0};
  for (uint32_t pass = 0; pass < (n + 63u) / 64u; ++pass) {
    Part p[64];
    bool head[64], has[64];
    Seg seg[64];
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      const uint32_t i = pass * 64u + lane;
      has[lane] = i < n;
      seg[lane] = seg_of(at, lane, W, N);
      cur[lane] = has[lane] ? word_of(r[lo + i].bid, r[lo + i].ask) : 0ull;
    }
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      const uint32_t i = pass * 64u + lane;
      const uint64_t prev = lane == 0u ? tail : cur[lane - 1u];
      const uint64_t bar = at.bar + seg[lane].rel;
      if (has[lane] && bar_start(bar, W) + seg[lane].phase != seen + i) return 3;  // the mapping names the step itself
      if (has[lane] && (bar != bar_of(seen + i, W) || seg[lane].slot != slot_of_bar(bar, N))) return 3;
      p[lane] = has[lane] ? term(seen + i, r[lo + i].tv, r[lo + i].bid, r[lo + i].ask, cur[lane], prev) : cleared();
      head[lane] = seg[lane].head || !has[lane];
    }
    tail = cur[63];
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
      Part q[64];
      bool q_head[64];
      for (uint32_t lane = 0; lane < 64u; ++lane) q[lane] = p[(lane - off) & 63u], q_head[lane] = head[(lane - off) & 63u];
      for (uint32_t lane = 0; lane < 64u; ++lane) scan_round(p[lane], head[lane], q[lane], q_head[lane], lane, off);
    }
    Part loaded[64];
    bool writes[64];
    std::vector<uint32_t> written;
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      const uint32_t i = pass * 64u + lane;
      writes[lane] = has[lane] && tail_of(seg[lane], lane, i, n, W) && !skipped(at.bar + seg[lane].rel, last_bar, N);
      if (writes[lane]) loaded[lane] = t.rows[seg[lane].slot];
    }
    for (uint32_t lane = 64u; lane-- > 0u;) {
      if (!writes[lane]) continue;
      for (uint32_t s : written)
        if (s == seg[lane].slot) return 4;  // two lanes of one pass on one slot: the result would depend on their order
      written.push_back(seg[lane].slot);
      t.rows[seg[lane].slot] = merged_row(loaded[lane], p[lane], at.bar + seg[lane].rel, W);
    }
    at = next_pass(at, W, N);
  }
  t.carry = cur[(n - 1u) & 63u];
  return 0;
}

static void fold_serial(Table& t, const std::vector<Rec>& r, uint64_t first, size_t lo, size_t hi) {
  uint64_t prev = t.carry;
  for (size_t s = lo; s < hi; ++s) {
    const uint64_t cur = word_of(r[s].bid, r[s].ask), bar = bar_of(first + s, t.W);
    Part& row = t.rows[slot_of_bar(bar, t.N)];
    row = merged_row(row, term(first + s, r[s].tv, r[s].bid, r[s].ask, cur, prev), bar, t.W);
    prev = cur;
  }
  t.carry = prev;
}

static void same(const Table& t, const std::vector<uint64_t>& w, const char* how, uint64_t series, uint64_t fold, int& bad) {
  for (uint32_t q = 0; q < t.N; ++q)
    for (uint32_t k = 0; k < ROW_WORDS; ++k)
      if (t.rows[q].w[k] != w[q * ROW_WORDS + k] && bad++ < 8)
        std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): slot %u word %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how,
                    q, k, t.rows[q].w[k], w[q * ROW_WORDS + k]);
  if (t.carry != w[t.N * ROW_WORDS] && bad++ < 8)
    std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): carry is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how, t.carry,
                w[t.N * ROW_WORDS]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* ex = std::fopen(argv[2], "r");
  if (!in || !ex) return 2;
  uint64_t n_series = 0, n_total = 0, n_folds_total = 0;
  if (std::fscanf(in, "%" SCNu64, &n_series) != 1) return 2;
  int bad = 0;
  for (uint64_t s = 0; s < n_series; ++s) {
    uint64_t n = 0, n_folds = 0, first = 0;
    uint32_t W = 0, N = 0;
    if (std::fscanf(in, "%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64, &n, &W, &N, &first, &n_folds) != 5) return 2;
    if (W < 1u || W > MAX_WIDTH || N < 1u || N > MAX_CANDLES) return 2;
    std::vector<uint64_t> ends(n_folds);
    std::vector<uint32_t> cuts(n_folds);
    for (uint64_t f = 0; f < n_folds; ++f)
      if (std::fscanf(in, "%" SCNu64 " %" SCNu32, &ends[f], &cuts[f]) != 2) return 2;
    std::vector<Rec> recs(n);
    for (Rec& r : recs)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32, &r.tv, &r.bid, &r.ask) != 3) return 2;
    Table lanes(W, N), serial(W, N);
    uint64_t lo = 0;
    std::vector<uint64_t> w(static_cast<size_t>(N) * ROW_WORDS + 1u);
    for (uint64_t f = 0; f < n_folds; ++f) {
      if (ends[f] <= lo || ends[f] > n) return 2;
      if (cuts[f]) lanes.carry = serial.carry = 0ull;
      if (int rc = fold_lanes(lanes, recs, first, lo, ends[f])) {
        std::printf("series %" PRIu64 " fold %" PRIu64 " (lanes): %s\n", s, f,
                    rc == 3 ? "the lane mapping names another step, bar or slot" : "two lanes of a pass write one slot");
        return 1;
      }
      fold_serial(serial, recs, first, lo, ends[f]);
      for (uint64_t& x : w)
        if (std::fscanf(ex, "%" SCNu64, &x) != 1) return 2;
      same(lanes, w, "lanes", s, f, bad);
      same(serial, w, "serial", s, f, bad);
      lo = ends[f];
    }
    n_total += n, n_folds_total += n_folds;
  }
  std::fclose(in);
  std::fclose(ex);
  if (bad) return 1;
  // the helpers on their own: bars and slots, the skipped bars of the issue's cases, continue or restart, the passes
  if (bar_of(0, 2) != 0u || bar_of(5, 2) != 2u || bar_of((1ull << 40) + 3u, MAX_WIDTH) != 1u << 20 || slot_of_bar(46, 4) != 2u) return 1;
  if (!skipped(0, 2, 2) || skipped(1, 2, 2) || skipped(2, 2, 2) || !skipped(41, 45, 4) || skipped(42, 45, 4)) return 1;
  Part row = cleared();
  if (continues(row, 0, 5)) return 1;  // n_steps == 0: first_step 0 is not a step of bar 0
  row.w[N_STEPS] = 1u, row.w[FIRST_STEP] = 13u;
  if (!continues(row, 2, 5) || continues(row, 3, 5) || continues(row, 1, 5) || continues(row, 2 + 3, 5)) return 1;
  row.w[FIRST_STEP] = 10u;
  if (!continues(row, 2, 5) || continues(row, 1, 5)) return 1;
  const uint32_t Ws[7] = {1, 3, 5, 64, 100, 7, MAX_WIDTH}, Ns[7] = {256, 4, 64, 4, 2, 1, 1};
  for (int c = 0; c < 7; ++c)
    for (uint64_t step : {0ull, 1ull, 63ull, 99ull, 1048575ull, 1048577ull, (1ull << 33) + 11ull}) {
      Pass at = first_pass(step, Ws[c], Ns[c]);
      for (uint32_t pass = 0; pass < 40u; ++pass) {
        const uint64_t s0 = step + 64ull * pass;
        if (at.bar != s0 / Ws[c] || at.phase != s0 % Ws[c] || at.slot != (s0 / Ws[c]) % Ns[c]) return 1;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
          const Seg g = seg_of(at, lane, Ws[c], Ns[c]);
          const uint64_t x = s0 + lane;
          if (at.bar + g.rel != x / Ws[c] || g.phase != x % Ws[c] || g.slot != (x / Ws[c]) % Ns[c]) return 1;
          if (g.head != (x % Ws[c] == 0u || lane == 0u)) return 1;
          if (tail_of(g, lane, 64u * pass + lane, 64u * 40u, Ws[c]) != (x % Ws[c] == Ws[c] - 1u || lane == 63u || (pass == 39u && lane == 63u))) return 1;
        }
        at = next_pass(at, Ws[c], Ns[c]);
      }
    }
  // one record: a return of 2^33 - 8 and its square modulo 2^64; a one-sided step adds its volume only
  const Part up = term(9, 7, 0xFFFFFFFDu, 0xFFFFFFFEu, word_of(0xFFFFFFFDu, 0xFFFFFFFEu), word_of(1, 2));
  const uint64_t a = (1ull << 33) - 8ull;
  if (up.w[FIRST_STEP] != 9u || up.w[OPEN_M] != (1ull << 33) - 5ull || up.w[SUM_SPREAD] != 1u || up.w[SUM_D] != a || up.w[SUM_D2] != a * a ||
      up.w[MAX_ABS_D] != a || up.w[N_TRADE_STEPS] != 1u || up.w[SUM_TRADE_VOL] != 7u)
    return 1;
  const Part one = term(10, 0xFFFFFFFFu, 0, 5, word_of(0, 5), word_of(1, 2));
  if (one.w[N_STEPS] != 1u || one.w[N_TWO_SIDED] || one.w[OPEN_M] || one.w[N_RET] || one.w[SUM_TRADE_VOL] != 0xFFFFFFFFull) return 1;
  const Part both = merge(one, up), other = merge(up, one);  // (not in step order: only the merge's rules are read)
  if (both.w[FIRST_STEP] != 10u || other.w[FIRST_STEP] != 9u || both.w[LOW_M] != up.w[LOW_M] || other.w[LOW_M] != up.w[LOW_M] ||
      both.w[CLOSE_M] != up.w[CLOSE_M] || other.w[CLOSE_M] != up.w[CLOSE_M] || both.w[N_STEPS] != 2u)
    return 1;
  std::printf("candle_fold ok %" PRIu64 " series %" PRIu64 " steps %" PRIu64 " folds\n", n_series, n_total, n_folds_total);
  return 0;
}
