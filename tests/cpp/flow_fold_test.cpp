// flow_fold_test.cpp - bourse_amd/csrc/flow_fold.hpp on the CPU, compiled plain and under the sanitizers (tests/test_flow_cpu.py).
//
// fold() below is the device fold (flow.hpp) lane by lane in plain C++: the window opens with the carry behind the front
// gap, records are taken CHUNK at a time, every "lane" k - 1 adds its pairs, the window's last K words move to the front, and
// the carry is taken behind the back gap.  Checked
//   1. against a double loop over all pairs of the tape;
//   2. for every way a tape is cut into folds (sizes 0, 1, 63, 64, 65, 130 among them, K larger than a fold): same words, carry;
//   3. with lost indices: gaps of 1, K - 1, K, K + 1 and 10^9 (which must not be walked);
// and with `dump` as its argument it reads a case from stdin and prints words, carry and cursor for the Python model.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bourse_amd/csrc/flow_fold.hpp"

using namespace bkd::flow;

struct Rec {
  uint32_t price, vol, side_is_bid;
};

struct Book {
  uint32_t K;
  std::vector<uint64_t> words, carry;  // 8 + 6 K, K
  uint64_t seen;
  explicit Book(uint32_t k, uint64_t at = 0) : K(k), words(table_words(k), 0), carry(k, 0), seen(at) {}
  void cut(uint64_t at) {
    carry.assign(K, 0);
    seen = at;
  }
};

static long g_walked = 0;  // records and gap indices fold() touched one by one

// tape(i): the record of index i (only called for readable indices)
template <typename Tape>
static void fold(Book& bk, const Tape& tape, uint64_t total, uint64_t base, uint64_t cap) {
  if (bk.seen >= total) return;
  const uint32_t K = bk.K;
  const Plan p = plan(bk.seen, total, base, cap);
  std::vector<uint64_t> win(WINDOW_WORDS, 0xDEADBEEFDEADBEEFull);
  for (uint32_t lane = 0; lane < K; ++lane) {
    const uint32_t src = carry_src(K, p.lost_front, lane);
    win[carry_at(K, lane)] = src == NO_ENTRY ? 0 : bk.carry[src];
  }
  Base sum{};
  std::vector<LagRow> acc(K, LagRow{});
  for (uint64_t c = p.lo; c < p.hi; c += CHUNK) {
    const uint32_t cnt = p.hi - c < CHUNK ? static_cast<uint32_t>(p.hi - c) : CHUNK;
    for (uint32_t lane = 0; lane < cnt; ++lane) {
      const Rec r = tape(c + lane);
      win[rec_at(K, lane)] = word_of(r.price, r.side_is_bid);
      add_record(sum, r.price, r.vol, r.side_is_bid);
      ++g_walked;
    }
    for (uint32_t i = 0; i < cnt; ++i)
      for (uint32_t lane = 0; lane < K; ++lane) add_pair(acc[lane], win[rec_at(K, i)], win[rec_at(K, i) - (lane + 1u)]);
    std::vector<uint64_t> front(K);
    for (uint32_t lane = 0; lane < K; ++lane) front[lane] = win[cnt + lane];
    for (uint32_t lane = 0; lane < K; ++lane) win[lane] = front[lane];
  }
  sum.w[N_LOST] = p.lost_front + p.lost_back;
  Base b;
  std::memcpy(b.w, bk.words.data(), sizeof b.w);
  merge(b, sum);
  std::memcpy(bk.words.data(), b.w, sizeof b.w);
  for (uint32_t lane = 0; lane < K; ++lane) {
    LagRow r;
    std::memcpy(r.w, &bk.words[BASE_WORDS + LAG_WORDS * lane], sizeof r.w);
    merge(r, acc[lane]);
    std::memcpy(&bk.words[BASE_WORDS + LAG_WORDS * lane], r.w, sizeof r.w);
  }
  std::vector<uint64_t> next(K);
  for (uint32_t lane = 0; lane < K; ++lane) {
    const uint32_t src = carry_src(K, p.lost_back, lane);
    next[lane] = src == NO_ENTRY ? 0 : win[carry_at(K, src)];
  }
  bk.carry = next;
  bk.seen = total;
}

// all pairs of a tape of which ok[i] says whether index i was read
static std::vector<uint64_t> brute(const std::vector<Rec>& t, const std::vector<char>& ok, uint32_t K) {
  std::vector<uint64_t> w(table_words(K), 0);
  for (size_t i = 0; i < t.size(); ++i) {
    if (!ok[i]) {
      w[N_LOST] += 1;
      continue;
    }
    const bool buy = t[i].side_is_bid == 0;
    w[N_TRADES] += 1, w[N_BUY] += buy, w[SUM_VOL] += t[i].vol, w[BUY_VOL] += buy ? t[i].vol : 0;
    w[SUM_VOL_SQ] += static_cast<uint64_t>(t[i].vol) * t[i].vol;
    w[NOTIONAL] += static_cast<uint64_t>(t[i].vol) * t[i].price;
    if (t[i].vol > w[MAX_VOL]) w[MAX_VOL] = t[i].vol;
    for (uint32_t k = 1; k <= K && k <= i; ++k) {
      if (!ok[i - k]) continue;
      const int64_t s = buy ? 1 : -1, sk = t[i - k].side_is_bid == 0 ? 1 : -1;
      const int64_t dp = static_cast<int64_t>(t[i].price) - static_cast<int64_t>(t[i - k].price);
      uint64_t* r = &w[BASE_WORDS + LAG_WORDS * (k - 1)];
      r[N_PAIRS] += 1;
      r[SUM_SS] += static_cast<uint64_t>(s * sk);
      r[SUM_RESP] += static_cast<uint64_t>(sk * dp);
      r[SUM_BACK] += static_cast<uint64_t>(s * dp);
      r[SUM_ABS_DP] += static_cast<uint64_t>(dp < 0 ? -dp : dp);
      r[SUM_DP2] += static_cast<uint64_t>(dp) * static_cast<uint64_t>(dp);
    }
  }
  return w;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return static_cast<uint32_t>(g_rng >> 32);
}

static std::vector<Rec> random_tape(size_t n, bool wide) {
  std::vector<Rec> t(n);
  for (Rec& r : t) {
    r.price = wide ? rnd() : 1000u + rnd() % 50u;
    r.vol = wide ? rnd() : 1u + rnd() % 100u;
    r.side_is_bid = rnd() % 3u == 0 ? (wide ? rnd() | 1u : 1u) : 0u;
  }
  return t;
}

static int g_cases = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);            \
      return 1;                                                      \
    }                                                                \
    ++g_cases;                                                       \
  } while (0)

static int self_test() {
  // 1 + 2: every K of interest, tapes long and short, cut in many ways
  const uint32_t Ks[] = {1, 2, 3, 5, 16, 63, 64};
  const size_t sizes[] = {0, 1, 63, 64, 65, 130};
  for (uint32_t K : Ks)
    for (int wide = 0; wide < 2; ++wide) {
      const std::vector<Rec> t = random_tape(400, wide != 0);
      const auto tape = [&](uint64_t i) { return t[i]; };
      const std::vector<char> all(t.size(), 1);
      const std::vector<uint64_t> want = brute(t, all, K);
      Book whole(K);
      fold(whole, tape, t.size(), 0, 1u << 30);
      CHECK(whole.words == want && whole.seen == t.size());
      for (uint32_t j = 0; j < K; ++j) CHECK(whole.carry[j] == word_of(t[t.size() - 1 - j].price, t[t.size() - 1 - j].side_is_bid));
      for (size_t first : sizes)
        for (size_t step : sizes) {  // a fold of `first`, then folds of `step` (0: a fold of nothing, then the rest)
          Book cut(K);
          uint64_t at = first;
          fold(cut, tape, at, 0, 1u << 30);
          fold(cut, tape, at, 0, 1u << 30);  // (nothing new: nothing changes)
          while (at < t.size()) {
            at = step ? (at + step < t.size() ? at + step : t.size()) : t.size();
            fold(cut, tape, at, 0, 1u << 30);
          }
          CHECK(cut.words == want && cut.carry == whole.carry && cut.seen == whole.seen);
        }
      for (int n = 0; n < 20; ++n) {  // random cuts
        Book cut(K);
        uint64_t at = 0;
        while (at < t.size()) {
          at += rnd() % 140u;
          if (at > t.size()) at = t.size();
          fold(cut, tape, at, 0, 1u << 30);
        }
        CHECK(cut.words == want && cut.carry == whole.carry);
      }
    }
  // 3: lost indices.  A tape of which a run [g0, g0 + gap) was consumed before the fold saw it (base moved past it) ...
  for (uint32_t K : {1u, 4u, 16u, 64u})
    for (uint64_t gap : {uint64_t(1), uint64_t(K - 1), uint64_t(K), uint64_t(K + 1)}) {
      if (gap == 0) continue;
      const std::vector<Rec> t = random_tape(300, false);
      const auto tape = [&](uint64_t i) { return t[i]; };
      const uint64_t g0 = 100;
      std::vector<char> ok(t.size(), 1);
      for (uint64_t i = g0; i < g0 + gap; ++i) ok[i] = 0;
      const std::vector<uint64_t> want = brute(t, ok, K);
      Book a(K);
      fold(a, tape, g0, 0, 1u << 30);
      fold(a, tape, t.size(), g0 + gap, 1u << 30);  // in front of the readable run
      CHECK(a.words == want && a.words[N_LOST] == gap);
      Book b(K);
      fold(b, tape, g0 + gap, 0, g0);  // ... or dropped beyond the capacity: behind the readable run
      CHECK(b.words[N_LOST] == gap && b.seen == g0 + gap);
      fold(b, tape, t.size(), g0 + gap, 1u << 30);
      CHECK(b.words == want && b.carry == a.carry);
      Book c(K);  // both at once: capacity 40 from base 50 in a fold over [0, 150), then the rest
      std::vector<char> ok2(t.size(), 1);
      for (uint64_t i = 0; i < 150; ++i) ok2[i] = i >= 50 && i < 90;
      fold(c, tape, 150, 50, 40);
      fold(c, tape, t.size(), 150, 1u << 30);
      CHECK(c.words == brute(t, ok2, K));
    }
  // ... and a gap of 10^9, on both sides of a short readable run: counted, not walked
  {
    const uint64_t G = 1000000000ull;
    const std::vector<Rec> t = random_tape(40, false);
    const auto tape = [&](uint64_t i) { return t[i - G]; };
    Book a(8);
    fold(a, [&](uint64_t i) { return t[i]; }, 10, 0, 1u << 30);
    g_walked = 0;
    fold(a, tape, 2 * G, G, 40);  // lost: [10, G) in front, [G + 40, 2 G) behind
    CHECK(g_walked == 40);
    CHECK(a.words[N_LOST] == (G - 10) + (G - 40) && a.words[N_TRADES] == 50 && a.seen == 2 * G);
    for (uint64_t c : a.carry) CHECK(c == 0);
    Book fresh(8);
    std::vector<Rec> tail(t.begin(), t.end());
    fold(fresh, [&](uint64_t i) { return tail[i]; }, 40, 0, 1u << 30);
    Book head(8);
    fold(head, [&](uint64_t i) { return t[i]; }, 10, 0, 1u << 30);
    for (uint32_t k = 0; k < 8; ++k)  // the pairs are those inside the two runs, none across
      CHECK(a.words[BASE_WORDS + LAG_WORDS * k + N_PAIRS] ==
            fresh.words[BASE_WORDS + LAG_WORDS * k + N_PAIRS] + head.words[BASE_WORDS + LAG_WORDS * k + N_PAIRS]);
  }
  // plan(): by hand
  {
    Plan p = plan(10, 30, 0, 16);
    CHECK(p.lo == 10 && p.hi == 16 && p.lost_front == 0 && p.lost_back == 14);
    p = plan(10, 30, 20, 16);
    CHECK(p.lo == 20 && p.hi == 30 && p.lost_front == 10 && p.lost_back == 0);
    p = plan(10, 30, 30, 16);
    CHECK(p.lo == 30 && p.hi == 30 && p.lost_front == 20 && p.lost_back == 0);
    p = plan(40, 30, 0, 16);
    CHECK(p.lo == 30 && p.hi == 30 && p.lost_front == 0 && p.lost_back == 0);
    p = plan(20, 30, 0, 16);
    CHECK(p.lo == 20 && p.hi == 20 && p.lost_front == 0 && p.lost_back == 10);
    CHECK(carry_src(4, 0, 3) == 3 && carry_src(4, 1, 0) == NO_ENTRY && carry_src(4, 1, 3) == 2 && carry_src(4, 4, 3) == NO_ENTRY &&
          carry_src(4, ~0ull, 0) == NO_ENTRY);
  }
  std::printf("flow_fold ok %d cases\n", g_cases);
  return 0;
}

// stdin: K n, n records "price vol side_is_bid", start, F, F folds "total base capacity cut" (cut: -1 none, else the count a
// reset behind the fold restores).  stdout: the words, the carry, the cursor, one line each.
static int dump() {
  unsigned K;
  size_t n;
  if (std::scanf("%u %zu", &K, &n) != 2) return 2;
  std::vector<Rec> t(n);
  for (Rec& r : t)
    if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &r.price, &r.vol, &r.side_is_bid) != 3) return 2;
  uint64_t start;
  size_t F;
  if (std::scanf("%" SCNu64 " %zu", &start, &F) != 2) return 2;
  Book bk(K, start);
  for (size_t f = 0; f < F; ++f) {
    uint64_t total, base, cap;
    long long cut;
    if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %lld", &total, &base, &cap, &cut) != 4) return 2;
    fold(bk, [&](uint64_t i) { return t[i]; }, total, base, cap);
    if (cut >= 0) bk.cut(static_cast<uint64_t>(cut));
  }
  for (uint64_t w : bk.words) std::printf("%" PRIu64 " ", w);
  std::printf("\n");
  for (uint64_t w : bk.carry) std::printf("%" PRIu64 " ", w);
  std::printf("\n%" PRIu64 "\n", bk.seen);
  return 0;
}

int main(int argc, char** argv) { return argc > 1 && !std::strcmp(argv[1], "dump") ? dump() : self_test(); }
