// CPU test of bourse_amd/csrc/series_fold.hpp (tests/test_series_cpu.py compiles and runs it): what one level-2 record adds
// to a book's row of series moments, the carry, and the combination of partial rows, over the series of <records file>,
// compared word for word with the rows of <expected file>, which tests/series_model.py printed.
//   records:  n_series, then per series one line "n_steps n_folds end_1 .. end_n_folds" (0 < end_1 < .. = n_steps: the
//             series is folded as [0, end_1), [end_1, end_2), ..) and one line per step: trade_vol bid ask ask_vol bid_vol
//   expected: per series and fold one line: the row's 24 words (unsigned) after that fold
// Every fold is done twice.  "lanes": as the device kernel does it - step s belongs to lane (s - first) % 64, whose values
// in front of s come from the records of s - 1 and s - 2 while those lie in the fold and from the row's carry words
// otherwise; the 64 lanes' rows are merged and added to the row, the carry is the last step's.  "serial": record by
// record with next().  Both must give the expected row.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/series_fold.hpp"

using namespace bkd::series;

struct Rec {
  uint32_t tv, bid, ask, ask_vol, bid_vol;
};

static Row fold_lanes(const Row& in, const std::vector<Rec>& r, size_t lo, size_t hi) {
  const Prev carry = unpack(in.w[CARRY_M], in.w[CARRY_D]);
  Row lanes[64];
  for (Row& l : lanes) l = cleared();
  Prev tail = carry;
  for (size_t s = lo; s < hi; ++s) {
    const size_t i = s - lo;
    Prev p = carry;
    if (i >= 1) {
      Prev before1 = carry;
      if (i >= 2) before1 = quotes_only(r[s - 2].bid, r[s - 2].ask);
      p = prev_of(r[s - 1].bid, r[s - 1].ask, before1);
    }
    const Term t = term(r[s].tv, r[s].bid, r[s].ask, r[s].ask_vol, r[s].bid_vol, p);
    add(lanes[i % 64], t);
    if (s + 1 == hi) tail = next(t);
  }
  Row sum = cleared();
  for (int l = 63; l >= 0; --l) merge(sum, lanes[l]);  // (any order: the wave's reduction has none)
  Row out = in;
  merge(out, sum);
  pack(out, tail);
  return out;
}

static Row fold_serial(const Row& in, const std::vector<Rec>& r, size_t lo, size_t hi) {
  Row out = in;
  Prev p = unpack(in.w[CARRY_M], in.w[CARRY_D]);
  for (size_t s = lo; s < hi; ++s) {
    const Term t = term(r[s].tv, r[s].bid, r[s].ask, r[s].ask_vol, r[s].bid_vol, p);
    add(out, t);
    p = next(t);
  }
  pack(out, p);
  return out;
}

static bool same(const Row& r, const uint64_t w[ROW_WORDS], const char* how, uint64_t series, uint64_t fold, int& bad) {
  bool ok = true;
  for (uint32_t i = 0; i < ROW_WORDS; ++i)
    if (r.w[i] != w[i]) {
      ok = false;
      if (bad++ < 8)
        std::printf("series %" PRIu64 " fold %" PRIu64 " (%s): word %u is %" PRIu64 ", expected %" PRIu64 "\n", series, fold, how, i,
                    r.w[i], w[i]);
    }
  return ok;
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
    if (std::fscanf(in, "%" SCNu64 " %" SCNu64, &n, &n_folds) != 2) return 2;
    std::vector<uint64_t> ends(n_folds);
    for (uint64_t& e : ends)
      if (std::fscanf(in, "%" SCNu64, &e) != 1) return 2;
    std::vector<Rec> recs(n);
    for (Rec& r : recs)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &r.tv, &r.bid, &r.ask, &r.ask_vol, &r.bid_vol) != 5)
        return 2;
    Row lanes = cleared(), serial = cleared();
    uint64_t lo = 0;
    for (uint64_t f = 0; f < n_folds; ++f) {
      if (ends[f] <= lo || ends[f] > n) return 2;
      lanes = fold_lanes(lanes, recs, lo, ends[f]);
      serial = fold_serial(serial, recs, lo, ends[f]);
      uint64_t w[ROW_WORDS];
      for (uint64_t& x : w)
        if (std::fscanf(ex, "%" SCNu64, &x) != 1) return 2;
      same(lanes, w, "lanes", q, f, bad);
      same(serial, w, "serial", q, f, bad);
      lo = ends[f];
    }
    n_total += n, n_folds_total += n_folds;
  }
  if (bad) return 1;
  // the helpers on their own: the 128-bit product and power, the carry words, the cleared row
  uint64_t lo = 0, hi = 0;
  mul_64x64(~0ull, ~0ull, lo, hi);
  if (lo != 1ull || hi != 0xFFFFFFFFFFFFFFFEull) return 1;
  pow4_mod128(0x1FFFFFFF8ull, lo, hi);  // (2^33 - 8)^4 = 2^12 (2^30 - 1)^4, which needs 132 bits
  if (lo != 0xFFFFF00000001000ull || hi != 0xFFFFFF00000005FFull) return 1;
  Row r = cleared();
  for (uint32_t i = 0; i < ROW_WORDS; ++i)
    if (r.w[i] != (i == MIN_M ? ~0ull : 0ull)) return 1;
  Prev p;
  p.have_m = 1, p.m = 0x1FFFFFFFCull, p.have_d = 1, p.d = -5;
  pack(r, p);
  if (r.w[CARRY_M] != (0xC000000000000000ull | 0x1FFFFFFFCull) || r.w[CARRY_D] != 0xFFFFFFFFFFFFFFFBull) return 1;
  const Prev back = unpack(r.w[CARRY_M], r.w[CARRY_D]);
  if (!back.have_m || !back.have_d || back.m != p.m || back.d != -5) return 1;
  if (two_sided(0, 5) || two_sided(5, NO_ASK) || !two_sided(1, 0xFFFFFFFEu)) return 1;
  std::printf("series_fold ok %" PRIu64 " series %" PRIu64 " steps %" PRIu64 " folds\n", n_series, n_total, n_folds_total);
  return 0;
}
