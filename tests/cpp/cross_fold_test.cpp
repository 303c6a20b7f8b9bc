// CPU test of bourse_amd/csrc/cross_fold.hpp (tests/test_cross_cpu.py compiles and runs it): what one step adds to each of a
// market's S * A * A cross rows, the windows and the carry, over the markets of <records file>, compared word for word with
// the rows and carry of <expected file>, which tests/cross_model.py printed.
//   records:  n_markets, then per market one line "n_steps A S span_1 .. span_S n_folds end_1 .. end_n_folds"
//             (0 < end_1 < .. = n_steps: the market is folded as [0, end_1), [end_1, end_2), ..) and one line per step:
//             bid ask of asset 0, bid ask of asset 1, ..
//   expected: per market and fold S * A * A lines of the row's 8 words (unsigned), unit by unit, and A lines of the asset's
//             2 * Hmax carry words after it
// Every fold is done twice.  "lanes": as the device kernel does it - A windows that open with the 2 * Hmax carry words, chunks
// of up to 64 steps appended to them, the chunk's steps walked in order with lane l adding to the accumulators of its units
// l, l + 64, l + 128, l + 192 from the five words of the two windows, the windows' last 2 * Hmax words moved to their front
// after a chunk and to the carry at the end.  "serial": step by step, a whole fold at a time, on the full series with the
// words in front of the fold taken from the carry.  Both must give the expected rows and carry.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/cross_fold.hpp"

using namespace bkd::cross;

struct Rec {
  uint32_t bid, ask;
};

struct Table {
  uint32_t A, S, Hmax;
  uint32_t spans[MAX_SPANS];
  std::vector<Row> rows;        // [S * A * A]
  std::vector<uint64_t> carry;  // [A][2 * Hmax]
  Table(uint32_t a, uint32_t s, const uint32_t* h) : A(a), S(s), Hmax(0) {
    for (uint32_t j = 0; j < MAX_SPANS; ++j) spans[j] = j < S ? h[j] : 0u;
    for (uint32_t j = 0; j < S; ++j) Hmax = std::max(Hmax, spans[j]);
    rows.assign(units(S, A), Row{});
    carry.assign(static_cast<size_t>(A) * carry_words(Hmax), 0ull);
  }
};

// recs[step * A + asset]
static void fold_lanes(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const uint32_t A = t.A, Hmax = t.Hmax, C = carry_words(Hmax), U = units(t.S, A);
  std::vector<uint64_t> win(static_cast<size_t>(A) * window_words(Hmax), 0xDEADull);
  for (uint32_t a = 0; a < A; ++a)
    for (uint32_t j = 0; j < C; ++j) win[window_at(Hmax, a) + carry_at(j)] = t.carry[a * C + j];
  std::vector<Row> acc(MAX_UNITS, Row{});  // lane l's rounds at l, l + 64, l + 128, l + 192
  for (size_t base = lo; base < hi; base += CHUNK) {
    const uint32_t cnt = hi - base < CHUNK ? static_cast<uint32_t>(hi - base) : CHUNK;
    for (uint32_t lane = 0; lane < cnt; ++lane)
      for (uint32_t a = 0; a < A; ++a) {
        const Rec& rec = r[(base + lane) * A + a];
        win[window_at(Hmax, a) + step_at(Hmax, lane)] = word_of(rec.bid, rec.ask);
      }
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint32_t at = step_at(Hmax, i);
      for (uint32_t lane = 0; lane < 64u; ++lane)
        for (uint32_t round = 0; round * 64u < U; ++round) {
          const uint32_t u = lane + 64u * round;
          if (u >= U) continue;
          const Unit q = unit_at(A, u);
          const uint32_t h = t.spans[q.j];
          const uint64_t* wa = win.data() + window_at(Hmax, q.a) + at;
          const uint64_t* wb = win.data() + window_at(Hmax, q.b) + at;
          add(acc[u], wa[0], *(wa - h), wb[0], *(wb - h), *(wb - 2 * h));
        }
    }
    for (uint32_t a = 0; a < A; ++a) {
      uint64_t* w = win.data() + window_at(Hmax, a);
      std::vector<uint64_t> front(C);
      for (uint32_t j = 0; j < C; ++j) front[j] = w[front_from(cnt, j)];
      for (uint32_t j = 0; j < C; ++j) w[j] = front[j];
    }
  }
  for (uint32_t u = 0; u < U; ++u) merge(t.rows[u], acc[u]);
  for (uint32_t a = 0; a < A; ++a)
    for (uint32_t j = 0; j < C; ++j) t.carry[a * C + j] = win[window_at(Hmax, a) + carry_at(j)];
}

static void fold_serial(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const uint32_t A = t.A, C = carry_words(t.Hmax);
  // asset a's word of step s: of the fold if s >= lo, else carry entry C - (lo - s) (0 beyond the carry's reach)
  auto word = [&](uint32_t a, int64_t s) -> uint64_t {
    if (s >= static_cast<int64_t>(lo)) return word_of(r[s * A + a].bid, r[s * A + a].ask);
    const int64_t back = static_cast<int64_t>(lo) - s;
    return back <= static_cast<int64_t>(C) ? t.carry[a * C + (C - back)] : 0ull;
  };
  for (size_t s = lo; s < hi; ++s)
    for (uint32_t j = 0; j < t.S; ++j)
      for (uint32_t a = 0; a < A; ++a)
        for (uint32_t b = 0; b < A; ++b) {
          const int64_t at = static_cast<int64_t>(s), h = t.spans[j];
          add(t.rows[unit_of(A, j, a, b)], word(a, at), word(a, at - h), word(b, at), word(b, at - h), word(b, at - 2 * h));
        }
  std::vector<uint64_t> next(t.carry.size());
  for (uint32_t a = 0; a < A; ++a)
    for (uint32_t j = 0; j < C; ++j) next[a * C + j] = word(a, static_cast<int64_t>(hi) - C + j);
  t.carry = next;
}

static void same(const Table& t, const std::vector<uint64_t>& w, const char* how, uint64_t market, uint64_t fold, int& bad) {
  const uint32_t U = units(t.S, t.A);
  for (uint32_t u = 0; u < U; ++u)
    for (uint32_t i = 0; i < ROW_WORDS; ++i)
      if (t.rows[u].w[i] != w[u * ROW_WORDS + i] && bad++ < 8)
        std::printf("market %" PRIu64 " fold %" PRIu64 " (%s): unit %u word %u is %" PRIu64 ", expected %" PRIu64 "\n", market, fold,
                    how, u, i, t.rows[u].w[i], w[u * ROW_WORDS + i]);
  for (size_t j = 0; j < t.carry.size(); ++j)
    if (t.carry[j] != w[U * ROW_WORDS + j] && bad++ < 8)
      std::printf("market %" PRIu64 " fold %" PRIu64 " (%s): carry %zu is %" PRIu64 ", expected %" PRIu64 "\n", market, fold, how, j,
                  t.carry[j], w[U * ROW_WORDS + j]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* ex = std::fopen(argv[2], "r");
  if (!in || !ex) return 2;
  uint64_t n_markets = 0, n_total = 0, n_folds_total = 0;
  if (std::fscanf(in, "%" SCNu64, &n_markets) != 1) return 2;
  int bad = 0;
  for (uint64_t q = 0; q < n_markets; ++q) {
    uint64_t n = 0, n_folds = 0;
    uint32_t A = 0, S = 0, spans[MAX_SPANS] = {0, 0, 0, 0};
    if (std::fscanf(in, "%" SCNu64 " %" SCNu32 " %" SCNu32, &n, &A, &S) != 3) return 2;
    if (A < 2 || A > MAX_ASSETS || S < 1 || S > MAX_SPANS) return 2;
    for (uint32_t j = 0; j < S; ++j)
      if (std::fscanf(in, "%" SCNu32, &spans[j]) != 1 || spans[j] < 1 || spans[j] > MAX_SPAN) return 2;
    if (std::fscanf(in, "%" SCNu64, &n_folds) != 1) return 2;
    std::vector<uint64_t> ends(n_folds);
    for (uint64_t& e : ends)
      if (std::fscanf(in, "%" SCNu64, &e) != 1) return 2;
    std::vector<Rec> recs(n * A);
    for (Rec& r : recs)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32, &r.bid, &r.ask) != 2) return 2;
    Table lanes(A, S, spans), serial(A, S, spans);
    uint64_t lo = 0;
    std::vector<uint64_t> w(units(S, A) * ROW_WORDS + lanes.carry.size());
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
  std::fclose(in);
  std::fclose(ex);
  if (bad) return 1;
  // the helpers on their own: where the carry and the steps stand, the unit mapping, one step's terms
  if (carry_words(64) != 128 || window_words(64) != 192 || window_at(64, 7) + step_at(64, 63) != 8 * 192 - 1) return 1;
  if (step_at(1, 0) != 2 || carry_at(1) != 1 || front_from(64, 0) != 64 || front_from(1, 127) != 128) return 1;
  if (units(4, 8) != MAX_UNITS || unit_of(8, 3, 7, 7) != 255 || unit_of(3, 1, 2, 0) != 15) return 1;
  for (uint32_t A = 2; A <= MAX_ASSETS; ++A)
    for (uint32_t u = 0; u < units(MAX_SPANS, A); ++u) {
      const Unit q = unit_at(A, u);
      if (q.j >= MAX_SPANS || q.a >= A || q.b >= A || unit_of(A, q.j, q.a, q.b) != u) return 1;
    }
  Row r{};
  add(r, 0ull, TWO | 5, TWO | 4, TWO | 3, TWO | 2);  // a one-sided step of a adds nothing
  add(r, TWO | 5, TWO | 4, TWO | 4, 0ull, TWO | 2);  // nor does one of b at s - h
  for (uint32_t i = 0; i < ROW_WORDS; ++i)
    if (r.w[i] != 0ull) return 1;
  add(r, TWO | 9, TWO | 4, 0ull, TWO | 7, TWO | 10);  // b one-sided at s: the lead term alone, x = 5, z = -3
  if (r.w[N] != 0 || r.w[N_LEAD] != 1 || r.w[SUM_LEAD] != static_cast<uint64_t>(-15)) return 1;
  add(r, TWO | 2, TWO | 9, TWO | 4, TWO | 7, 0ull);  // x = -7, y = -3, no lead
  if (r.w[N] != 1 || r.w[SUM_X] != static_cast<uint64_t>(-7) || r.w[SUM_Y] != static_cast<uint64_t>(-3) || r.w[SUM_XX] != 49 ||
      r.w[SUM_YY] != 9 || r.w[SUM_XY] != 21 || r.w[N_LEAD] != 1)
    return 1;
  std::printf("cross_fold ok %" PRIu64 " markets %" PRIu64 " steps %" PRIu64 " folds\n", n_markets, n_total, n_folds_total);
  return 0;
}
