// CPU test of bourse_amd/csrc/bin_fold.hpp (tests/test_bins_cpu.py compiles and runs it): which bin one level-2 record
// raises in every channel of a book's bin table, where a span's partner stands and how the carry moves on, over the series
// of <records file>, compared word for word with the counts and carry of <expected file>, which tests/bins_model.py printed.
//   records:  n_series, then per series one line "n_steps B S k_0 .. k_{S-1} ret_width spread_width vol_width n_folds
//             end_1 .. end_n_folds" (0 < end_1 < .. = n_steps: the series is folded as [0, end_1), [end_1, end_2), ..) and
//             one line per step: trade_vol bid ask
//   expected: per series and fold S + 2 lines of B counts and one line of the Kmax carry words after it
// Every fold is done twice.  "lanes": as the device kernel does it - a block of (S + 2) x B u32 counters zeroed first, 64
// lanes of which lane l takes steps l, l + 64, .. of the fold, each reading its span partners from the fold's own records
// (the ring) or from the carry as partner() says, the non-zero counters then added to the u64 table, and every carry entry
// built from next_carry() before any is written.  "serial": record by record on the full series, with the words in front of
// the fold taken from the carry.  Both must give the expected counts and carry.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/bin_fold.hpp"

using namespace bkd::bins;

struct Rec {
  uint32_t tv, bid, ask;
};

struct Cfg {
  uint32_t B, S, k[MAX_SPANS], rw, sw, vw, Kmax;
};

struct Table {
  Cfg c;
  std::vector<uint64_t> counts;  // [S + 2][B]
  std::vector<uint64_t> carry;   // [Kmax]
  explicit Table(const Cfg& cfg) : c(cfg), counts((cfg.S + 2u) * cfg.B, 0ull), carry(cfg.Kmax, 0ull) {}
};

static void fold_lanes(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const Cfg& c = t.c;
  const uint32_t n = static_cast<uint32_t>(hi - lo), B = c.B, S = c.S;
  std::vector<uint32_t> cnt((S + 2u) * B, 0u);
  for (uint32_t lane = 0; lane < 64u; ++lane)
    for (uint32_t i = lane; i < n; i += 64u) {
      const Rec& x = r[lo + i];
      const uint64_t cur = word_of(x.bid, x.ask);
      cnt[(S + 1u) * B + vol_bin(x.tv, c.vw, B)] += 1u;
      if (!(cur & TWO)) continue;
      cnt[S * B + spread_bin(x.bid, x.ask, c.sw, B)] += 1u;
      for (uint32_t j = 0; j < S; ++j) {
        const Where w = partner(i, c.k[j]);
        const uint64_t at_k = w.in_ring ? word_of(r[lo + w.at].bid, r[lo + w.at].ask) : t.carry[w.at];
        if (at_k & TWO) cnt[j * B + ret_bin(cur, at_k, c.rw, B)] += 1u;
      }
    }
  for (size_t v = 0; v < cnt.size(); ++v)
    if (cnt[v]) t.counts[v] += cnt[v];
  std::vector<uint64_t> next(c.Kmax);
  for (uint32_t i = 0; i < c.Kmax; ++i) {
    const Where w = next_carry(n, i);
    next[i] = w.in_ring ? word_of(r[lo + w.at].bid, r[lo + w.at].ask) : t.carry[w.at];
  }
  t.carry = next;
}

static void fold_serial(Table& t, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const Cfg& c = t.c;
  // the word of step s: of the fold if s >= lo, else carry entry lo - 1 - s
  auto word = [&](int64_t s) -> uint64_t {
    if (s >= static_cast<int64_t>(lo)) return word_of(r[s].bid, r[s].ask);
    const int64_t i = static_cast<int64_t>(lo) - 1 - s;
    return i < static_cast<int64_t>(c.Kmax) ? t.carry[i] : 0ull;
  };
  for (size_t s = lo; s < hi; ++s) {
    const uint64_t cur = word(static_cast<int64_t>(s));
    t.counts[(c.S + 1u) * c.B + vol_bin(r[s].tv, c.vw, c.B)] += 1u;
    if (!(cur & TWO)) continue;
    t.counts[c.S * c.B + spread_bin(r[s].bid, r[s].ask, c.sw, c.B)] += 1u;
    for (uint32_t j = 0; j < c.S; ++j) {
      const uint64_t at_k = word(static_cast<int64_t>(s) - c.k[j]);
      if (at_k & TWO) t.counts[j * c.B + ret_bin(cur, at_k, c.rw, c.B)] += 1u;
    }
  }
  std::vector<uint64_t> next(c.Kmax);
  for (uint32_t i = 0; i < c.Kmax; ++i) next[i] = word(static_cast<int64_t>(hi) - 1 - i);
  t.carry = next;
}

static void same(const Table& t, const std::vector<uint64_t>& w, const char* how, uint64_t series, uint64_t fold, int& bad) {
  const uint32_t CB = (t.c.S + 2u) * t.c.B;
  for (uint32_t v = 0; v < CB; ++v)
    if (t.counts[v] != w[v] && bad++ < 8)
      std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): channel %u bin %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold,
                  how, v / t.c.B, v % t.c.B, t.counts[v], w[v]);
  for (uint32_t i = 0; i < t.c.Kmax; ++i)
    if (t.carry[i] != w[CB + i] && bad++ < 8)
      std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): carry %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how, i,
                  t.carry[i], w[CB + i]);
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
    Cfg c{};
    if (std::fscanf(in, "%" SCNu64 " %" SCNu32 " %" SCNu32, &n, &c.B, &c.S) != 3) return 2;
    if (c.B < 2 || c.B > MAX_BINS || c.B % 2 || c.S < 1 || c.S > MAX_SPANS) return 2;
    for (uint32_t j = 0; j < c.S; ++j) {
      if (std::fscanf(in, "%" SCNu32, &c.k[j]) != 1 || c.k[j] < 1 || c.k[j] > MAX_SPAN) return 2;
      c.Kmax = c.k[j] > c.Kmax ? c.k[j] : c.Kmax;
    }
    if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64, &c.rw, &c.sw, &c.vw, &n_folds) != 4) return 2;
    if (!c.rw || !c.sw || !c.vw) return 2;
    std::vector<uint64_t> ends(n_folds);
    for (uint64_t& e : ends)
      if (std::fscanf(in, "%" SCNu64, &e) != 1) return 2;
    std::vector<Rec> recs(n);
    for (Rec& r : recs)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32, &r.tv, &r.bid, &r.ask) != 3) return 2;
    Table lanes(c), serial(c);
    uint64_t lo = 0;
    std::vector<uint64_t> w((c.S + 2u) * c.B + c.Kmax);
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
  // the helpers on their own: the floor, the three bin rules, where a partner and a carry entry stand, the ring slot
  if (floor_div(-1, 3) != -1 || floor_div(-3, 3) != -1 || floor_div(-4, 3) != -2 || floor_div(0, 3) != 0 || floor_div(5, 3) != 1) return 1;
  if (floor_div(-(1ll << 33) + 8, 0xFFFFFFFFu) != -2 || floor_div((1ll << 33) - 8, 0xFFFFFFFFu) != 1 || floor_div(-7, 1) != -7) return 1;
  const uint64_t at = TWO | 100ull;
  if (ret_bin(TWO | 99ull, at, 3, 8) != 3 || ret_bin(TWO | 97ull, at, 3, 8) != 3 || ret_bin(TWO | 96ull, at, 3, 8) != 2) return 1;
  if (ret_bin(TWO | 100ull, at, 3, 8) != 4 || ret_bin(TWO | 111ull, at, 3, 8) != 7 || ret_bin(TWO | 1000ull, at, 3, 8) != 7) return 1;
  if (ret_bin(TWO | 88ull, at, 3, 8) != 0 || ret_bin(TWO | 1ull, at, 3, 8) != 0) return 1;
  if (ret_bin(word_of(0xFFFFFFFDu, 0xFFFFFFFEu), word_of(1, 2), 1, 256) != 255 || ret_bin(word_of(1, 2), word_of(0xFFFFFFFDu, 0xFFFFFFFEu), 1, 256) != 0)
    return 1;
  if (spread_bin(10, 17, 2, 64) != 3 || spread_bin(10, 9, 1, 64) != 63 || spread_bin(1, 0xFFFFFFFEu, 0xFFFFFFFFu, 2) != 0) return 1;
  if (vol_bin(0, 7, 4) != 0 || vol_bin(6, 7, 4) != 0 || vol_bin(7, 7, 4) != 1 || vol_bin(0xFFFFFFFFu, 1, 256) != 255) return 1;
  if (!partner(5, 5).in_ring || partner(5, 5).at != 0 || partner(4, 5).in_ring || partner(4, 5).at != 0 || partner(0, 64).at != 63) return 1;
  if (!next_carry(3, 2).in_ring || next_carry(3, 2).at != 0 || next_carry(3, 3).in_ring || next_carry(3, 3).at != 0 || next_carry(1, 63).at != 62)
    return 1;
  if (slot_of(5, 2, 8) != 7 || slot_of(5, 3, 8) != 0 || slot_of(7, 7, 8) != 6 || slot_of(0xFFFFFFFEu, 0xFFFFFFFEu, 0xFFFFFFFFull) != 0xFFFFFFFDull)
    return 1;
  std::printf("bin_fold ok %" PRIu64 " series %" PRIu64 " steps %" PRIu64 " folds\n", n_series, n_total, n_folds_total);
  return 0;
}
