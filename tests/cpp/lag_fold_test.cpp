// CPU test of bourse_amd/csrc/lag_fold.hpp (tests/test_lags_cpu.py compiles and runs it): what one level-2 record adds to
// each of a book's K lag rows, the window and the carry, over the series of <records file>, compared word for word with the
// rows and carry of <expected file>, which tests/lags_model.py printed.
//   records:  n_series, then per series one line "n_steps K n_folds end_1 .. end_n_folds" (0 < end_1 < .. = n_steps: the
//             series is folded as [0, end_1), [end_1, end_2), ..) and one line per step: bid ask
//   expected: per series and fold K lines of the row's 10 words (unsigned) and one line of the K + 1 carry words after it
// Every fold is done twice.  "lanes": as the device kernel does it - a window that opens with the K + 1 carry words, chunks
// of up to 64 steps appended to it, the chunk's steps walked in order with lane k - 1 reading the words of s - k and
// s - k - 1 from the window and adding to its own row, the window's last K + 1 words moved to its front after a chunk and
// to the carry at the end.  "serial": record by record, a whole fold at a time, on the full series with the words in front
// of the start taken from the carry.  Both must give the expected rows and carry.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/lag_fold.hpp"

using namespace bkd::lags;

struct Rec {
  uint32_t bid, ask;
};

struct Table {
  uint32_t K;
  std::vector<Row> rows;        // [K]
  std::vector<uint64_t> carry;  // [K + 1]
  explicit Table(uint32_t k) : K(k), rows(k, Row{}), carry(k + 1, 0ull) {}
};

static void fold_lanes(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const uint32_t K = t.K;
  uint64_t win[WINDOW_WORDS];
  for (uint32_t j = 0; j <= K; ++j) win[carry_at(K, j)] = t.carry[j];
  std::vector<Row> acc(K, Row{});
  for (size_t base = lo; base < hi; base += CHUNK) {
    const uint32_t cnt = hi - base < CHUNK ? static_cast<uint32_t>(hi - base) : CHUNK;
    uint64_t mine[CHUNK] = {};
    for (uint32_t lane = 0; lane < cnt; ++lane) {
      mine[lane] = word_of(r[base + lane].bid, r[base + lane].ask);
      win[step_at(K, lane)] = mine[lane];
    }
    uint64_t prev = win[carry_at(K, 0)];
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint64_t cur = mine[i];
      for (uint32_t lane = 0; lane < K; ++lane) {
        const uint32_t at = step_at(K, i) - (lane + 1u);
        add(acc[lane], cur, prev, win[at], win[at - 1u]);
      }
      prev = cur;
    }
    uint64_t front[MAX_LAGS + 1u];
    for (uint32_t j = 0; j <= K; ++j) front[j] = win[cnt + j];
    for (uint32_t j = 0; j <= K; ++j) win[j] = front[j];
  }
  for (uint32_t lane = 0; lane < K; ++lane) merge(t.rows[lane], acc[lane]);
  for (uint32_t j = 0; j <= K; ++j) t.carry[j] = win[carry_at(K, j)];
}

static void fold_serial(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const uint32_t K = t.K;
  // the word of step s: of the fold if s >= lo, else carry entry lo - 1 - s (0 beyond the carry's reach)
  auto word = [&](int64_t s) -> uint64_t {
    if (s >= static_cast<int64_t>(lo)) return word_of(r[s].bid, r[s].ask);
    const int64_t j = static_cast<int64_t>(lo) - 1 - s;
    return j <= static_cast<int64_t>(K) ? t.carry[j] : 0ull;
  };
  for (size_t s = lo; s < hi; ++s)
    for (uint32_t k = 1; k <= K; ++k)
      add(t.rows[k - 1], word(s), word(static_cast<int64_t>(s) - 1), word(static_cast<int64_t>(s) - k),
          word(static_cast<int64_t>(s) - k - 1));
  std::vector<uint64_t> next(K + 1);
  for (uint32_t j = 0; j <= K; ++j) next[j] = word(static_cast<int64_t>(hi) - 1 - j);
  t.carry = next;
}

static void same(const Table& t, const std::vector<uint64_t>& w, const char* how, uint64_t series, uint64_t fold, int& bad) {
  for (uint32_t k = 0; k < t.K; ++k)
    for (uint32_t i = 0; i < ROW_WORDS; ++i)
      if (t.rows[k].w[i] != w[k * ROW_WORDS + i] && bad++ < 8)
        std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): lag %u word %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold,
                    how, k + 1, i, t.rows[k].w[i], w[k * ROW_WORDS + i]);
  for (uint32_t j = 0; j <= t.K; ++j)
    if (t.carry[j] != w[t.K * ROW_WORDS + j] && bad++ < 8)
      std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): carry %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how, j,
                  t.carry[j], w[t.K * ROW_WORDS + j]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* ex = std::fopen(argv[2], "r");
  if (!in || !ex) return 2;
  uint64_t n_series = 0, n_total = 0, n_folds_total = 0;
  if (std::fscanf(in, "%" SCNu64, &n_series) != 1) return 2;
  int bad = 0;
  for (uint64_t q = 0; q < n_series; ++q) {
    uint64_t n = 0, n_folds = 0;
    uint32_t K = 0;
    if (std::fscanf(in, "%" SCNu64 " %" SCNu32 " %" SCNu64, &n, &K, &n_folds) != 3) return 2;
    if (K < 1 || K > MAX_LAGS) return 2;
    std::vector<uint64_t> ends(n_folds);
    for (uint64_t& e : ends)
      if (std::fscanf(in, "%" SCNu64, &e) != 1) return 2;
    std::vector<Rec> recs(n);
    for (Rec& r : recs)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32, &r.bid, &r.ask) != 2) return 2;
    Table lanes(K), serial(K);
    uint64_t lo = 0;
    std::vector<uint64_t> w(K * ROW_WORDS + K + 1);
    for (uint64_t f = 0; f < n_folds; ++f) {
      if (ends[f] <= lo || ends[f] > n) return 2;
      fold_lanes(lanes, recs, lo, ends[f]);
      fold_serial(serial, recs, lo, ends[f]);
      for (uint64_t& x : w)
        if (std::fscanf(ex, "%" SCNu64, &x) != 1) return 2;
      same(lanes, w, "lanes", q, f, bad);
      same(serial, w, "serial", q, f, bad);
      lo = ends[f];
    }
    n_total += n, n_folds_total += n_folds;
  }
  if (bad) return 1;
  // the helpers on their own: the window word and where the carry and the steps stand
  if (word_of(0, 5) != 0ull || word_of(5, 0xFFFFFFFFu) != 0ull || word_of(1, 0xFFFFFFFEu) != (TWO | 0xFFFFFFFFull)) return 1;
  if (word_of(0xFFFFFFFDu, 0xFFFFFFFEu) != (TWO | 0x1FFFFFFFBull)) return 1;
  if (carry_at(64, 0) != 64 || carry_at(64, 64) != 0 || step_at(64, 63) != WINDOW_WORDS - 1 || step_at(1, 0) != 2) return 1;
  Row r{};
  add(r, 0ull, TWO | 5, TWO | 4, TWO | 3);  // a one-sided step adds nothing
  for (uint32_t i = 0; i < ROW_WORDS; ++i)
    if (r.w[i] != 0ull) return 1;
  add(r, TWO | 9, 0ull, TWO | 4, TWO | 3);  // a span without a return at s: no pair
  if (r.w[N_H] != 1 || r.w[SUM_H] != 5 || r.w[SUM_H4_LO] != 625 || r.w[N_PAIRS] != 0) return 1;
  add(r, TWO | 2, TWO | 9, TWO | 4, TWO | 7);  // d = -7, d_k = -3
  if (r.w[N_H] != 2 || r.w[SUM_H] != 3 || r.w[SUM_ABS_H] != 7 || r.w[MAX_ABS_H] != 5 || r.w[N_PAIRS] != 1 || r.w[SUM_DD] != 21 ||
      r.w[SUM_ABS_DD] != 21)
    return 1;
  std::printf("lag_fold ok %" PRIu64 " series %" PRIu64 " steps %" PRIu64 " folds\n", n_series, n_total, n_folds_total);
  return 0;
}
