// CPU test of bourse_amd/csrc/depth_fold.hpp (tests/test_depth_cpu.py compiles and runs it): what one level of one level-2
// record adds to its row of a book's depth table, what the record adds to the header, and which lane of the device fold
// reads which (step, level), over the series of <records file>, compared word for word with the rows and carry of
// <expected file>, which tests/depth_model.py printed.
//   records:  n_series, then per series one line "n_steps L n_folds end_1 .. end_n_folds" (0 < end_1 < .. = n_steps: the
//             series is folded as [0, end_1), [end_1, end_2), ..) and one line per step: bid ask, then bid_vol bid_n ask_vol
//             ask_n per level
//   expected: per series and fold L + 1 lines of 16 words and one line of the L + 1 carry words after it
// Every fold is done twice.  "lanes": as the device kernel does it - 64 lanes, lane g * Lp + q on level q of step
// pass * G + g, the cumulative imbalance by a segmented scan over the Lp lanes of a group (each round reads the round
// before of the lane `off` below), the imbalance of the step before from lane - Lp, for group 0 from the last group of the
// pass before, for the first step from the carry; sixteen sums per lane, the groups added by xor rounds, group 0 added to
// the rows, the carry from the lanes of the last step.  "serial": step by step and level by level, the step in front of the
// fold from the carry.  Both must give the expected rows and carry.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/depth_fold.hpp"

using namespace bkd::depth;

struct Rec {
  uint32_t bid, ask;
  std::vector<uint32_t> lv;  // [L][4]
};

struct Table {
  uint32_t L;
  std::vector<Row> rows;        // [L + 1], the last the header
  std::vector<uint64_t> carry;  // [L + 1]
  explicit Table(uint32_t levels) : L(levels), rows(levels + 1u, cleared()), carry(levels + 1u, 0ull) {}
};

static void fold_lanes(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const uint32_t n = static_cast<uint32_t>(hi - lo), L = t.L;
  const Lanes a = lanes_of(L);
  int64_t tail[64], I[64] = {0};
  uint64_t cur[64] = {0};
  Row acc[64], hdr[64];
  for (uint32_t lane = 0; lane < 64u; ++lane) {
    const uint32_t q = level_of(a, lane);
    tail[lane] = q < L ? static_cast<int64_t>(t.carry[q]) : 0;
    acc[lane] = cleared(), hdr[lane] = cleared();
  }
  const uint64_t carry_word = t.carry[L];
  for (uint32_t pass = 0; pass < passes_of(a, n); ++pass) {
    uint32_t bid[64], ask[64], lv[64][4];
    uint64_t prev[64];
    bool has[64];
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      const uint32_t q = level_of(a, lane), i = step_of(a, pass, lane);
      has[lane] = i < n;
      bid[lane] = ask[lane] = 0u;
      lv[lane][0] = lv[lane][1] = lv[lane][2] = lv[lane][3] = 0u;
      prev[lane] = 0ull;
      if (has[lane]) {
        const Rec& x = r[lo + i];
        bid[lane] = x.bid, ask[lane] = x.ask;
        if (q < L)
          for (uint32_t k = 0; k < 4u; ++k) lv[lane][k] = x.lv[level_at(q) - REC_HEAD + k];
        prev[lane] = i >= 1u ? word_of(r[lo + i - 1u].bid, r[lo + i - 1u].ask) : carry_word;
      }
      cur[lane] = has[lane] ? word_of(bid[lane], ask[lane]) : 0ull;
      I[lane] = static_cast<int64_t>(static_cast<uint64_t>(lv[lane][0]) - static_cast<uint64_t>(lv[lane][2]));
    }
    for (uint32_t off = 1u; off < a.Lp; off <<= 1) {
      int64_t below[64];
      for (uint32_t lane = 0; lane < 64u; ++lane) below[lane] = I[(lane - off) & 63u];
      for (uint32_t lane = 0; lane < 64u; ++lane)
        if (level_of(a, lane) >= off) I[lane] = static_cast<int64_t>(static_cast<uint64_t>(I[lane]) + static_cast<uint64_t>(below[lane]));
    }
    int64_t J[64], next_tail[64];
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      J[lane] = group_of(a, lane) == 0u ? tail[lane] : I[(lane - a.Lp) & 63u];
      next_tail[lane] = I[tail_lane(a, level_of(a, lane))];
    }
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      tail[lane] = next_tail[lane];
      if (!has[lane]) continue;
      add_level(acc[lane], lv[lane][0], lv[lane][1], lv[lane][2], lv[lane][3], I[lane], J[lane], cur[lane], prev[lane]);
      add_header(hdr[lane], bid[lane], ask[lane], cur[lane], prev[lane]);
    }
  }
  std::vector<uint64_t> next(L + 1u);
  for (uint32_t q = 0; q < L; ++q) next[q] = static_cast<uint64_t>(I[last_lane(a, n, q)]);
  next[L] = cur[last_lane(a, n, 0u)];
  for (uint32_t off = a.Lp; off < 64u; off <<= 1) {
    Row other_acc[64], other_hdr[64];
    for (uint32_t lane = 0; lane < 64u; ++lane) other_acc[lane] = acc[lane ^ off], other_hdr[lane] = hdr[lane ^ off];
    for (uint32_t lane = 0; lane < 64u; ++lane) merge(acc[lane], other_acc[lane]), merge(hdr[lane], other_hdr[lane]);
  }
  for (uint32_t q = 0; q < L; ++q) merge(t.rows[q], acc[q]);  // the lanes of group 0
  merge(t.rows[L], hdr[0]);
  t.carry = next;
}

static void fold_serial(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const uint32_t L = t.L;
  std::vector<int64_t> before(L), now(L);
  for (uint32_t q = 0; q < L; ++q) before[q] = static_cast<int64_t>(t.carry[q]);
  uint64_t prev = t.carry[L];
  for (size_t s = lo; s < hi; ++s) {
    const Rec& x = r[s];
    const uint64_t cur = word_of(x.bid, x.ask);
    uint64_t run = 0ull;
    for (uint32_t q = 0; q < L; ++q) {
      const uint32_t* lv = &x.lv[level_at(q) - REC_HEAD];
      run += static_cast<uint64_t>(lv[0]) - static_cast<uint64_t>(lv[2]);
      now[q] = static_cast<int64_t>(run);
      add_level(t.rows[q], lv[0], lv[1], lv[2], lv[3], now[q], before[q], cur, prev);
    }
    add_header(t.rows[L], x.bid, x.ask, cur, prev);
    before = now;
    prev = cur;
  }
  for (uint32_t q = 0; q < L; ++q) t.carry[q] = static_cast<uint64_t>(before[q]);
  t.carry[L] = prev;
}

static void same(const Table& t, const std::vector<uint64_t>& w, const char* how, uint64_t series, uint64_t fold, int& bad) {
  for (uint32_t q = 0; q <= t.L; ++q)
    for (uint32_t k = 0; k < ROW_WORDS; ++k)
      if (t.rows[q].w[k] != w[q * ROW_WORDS + k] && bad++ < 8)
        std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): row %u word %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how,
                    q, k, t.rows[q].w[k], w[q * ROW_WORDS + k]);
  for (uint32_t i = 0; i <= t.L; ++i)
    if (t.carry[i] != w[(t.L + 1u) * ROW_WORDS + i] && bad++ < 8)
      std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): carry %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how, i,
                  t.carry[i], w[(t.L + 1u) * ROW_WORDS + i]);
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
    uint64_t n = 0, n_folds = 0;
    uint32_t L = 0;
    if (std::fscanf(in, "%" SCNu64 " %" SCNu32 " %" SCNu64, &n, &L, &n_folds) != 3) return 2;
    if (L < 1u || L > MAX_LEVELS) return 2;
    std::vector<uint64_t> ends(n_folds);
    for (uint64_t& e : ends)
      if (std::fscanf(in, "%" SCNu64, &e) != 1) return 2;
    std::vector<Rec> recs(n);
    for (Rec& r : recs) {
      r.lv.resize(4u * L);
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32, &r.bid, &r.ask) != 2) return 2;
      for (uint32_t& x : r.lv)
        if (std::fscanf(in, "%" SCNu32, &x) != 1) return 2;
    }
    Table lanes(L), serial(L);
    uint64_t lo = 0;
    std::vector<uint64_t> w((L + 1u) * ROW_WORDS + L + 1u);
    for (uint64_t f = 0; f < n_folds; ++f) {
      if (ends[f] <= lo || ends[f] > n) return 2;
      fold_lanes(lanes, recs, lo, ends[f]);
      fold_serial(serial, recs, lo, ends[f]);
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
  // the helpers on their own: the lanes' division, the last step's lanes, where a level stands, a pair and its move
  const uint32_t Ls[8] = {1, 2, 5, 16, 31, 32, 33, 64}, Lps[8] = {1, 2, 8, 16, 32, 32, 64, 64};
  for (int i = 0; i < 8; ++i) {
    const Lanes a = lanes_of(Ls[i]);
    if (a.Lp != Lps[i] || (1u << a.shift) != a.Lp || a.G * a.Lp != 64u) return 1;
    if (passes_of(a, 1) != 1u || passes_of(a, a.G) != 1u || passes_of(a, a.G + 1u) != 2u || passes_of(a, 200) != (200u + a.G - 1u) / a.G) return 1;
    if (step_of(a, 3, 63) != 3u * a.G + a.G - 1u || level_of(a, 63) != a.Lp - 1u || group_of(a, 0) != 0u) return 1;
    if (last_lane(a, 1, 0) != 0u || last_lane(a, a.G, 0) != 64u - a.Lp || last_lane(a, a.G + 1u, a.Lp - 1u) != a.Lp - 1u) return 1;
    if (tail_lane(a, 0) != 64u - a.Lp) return 1;
  }
  if (level_at(0) != 5u || level_at(63) != 257u) return 1;
  if (!pair_of(TWO | 5ull, TWO | 9ull) || pair_of(TWO | 5ull, 0ull) || pair_of(0ull, TWO | 9ull) || move_of(TWO | 5ull, TWO | 9ull) != -4) return 1;
  if (move_of(word_of(0xFFFFFFFDu, 0xFFFFFFFEu), word_of(1, 2)) != (1ll << 33) - 8) return 1;
  std::printf("depth_fold ok %" PRIu64 " series %" PRIu64 " steps %" PRIu64 " folds\n", n_series, n_total, n_folds_total);
  return 0;
}
