// agent_rows.hpp (the one text of an entry's checks and record arithmetic: host installs, host retunes, retune kernels)
// compiled with g++.  For a few thousand random rows and every edge row:
//   * the record and the status equal what make_groups / make_mixed_descs (agent_table.hpp) give for the same row.  The
//     builders delegate to agent_rows.hpp, so this holds the wiring (assets, ticks, the fixed-slot count, messages) and NOT
//     the arithmetic: it compares the shared text with itself;
//   * what pins the arithmetic and the checks is the rest - keep it: the status equals a predicate written out here
//     (expect_group / expect_member), in the header's terms (bk_random_agents / bk_agent_desc fields), the record's fields
//     equal the row's, and tests/cpp/per_book_table_test.cpp / members_per_book_table_test.cpp hold the builders' records;
//   * the thresholds equal the floating-point comparisons they replace, at the draws around them;
//   * the retune's fixed-field checks refuse a changed n_agents, type or agent_id_start and nothing else.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../bourse_amd/csrc/agent_table.hpp"

using namespace bkd;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// gen::<f32>() of the draw k = (u32 >> 8)
static float draw(uint32_t k) { return static_cast<float>(k) * (1.0f / 16777216.0f); }

static void check_rate(float rate, uint32_t thr) {  // (k < thr) <=> (draw(k) < rate) at the draws around thr
  for (int d = -2; d <= 2; ++d) {
    const int64_t k = static_cast<int64_t>(thr) + d;
    if (k < 0 || k >= (1 << 24)) continue;
    CHECK((static_cast<uint32_t>(k) < thr) == (draw(static_cast<uint32_t>(k)) < rate));
  }
  CHECK((0u < thr) == (draw(0) < rate));
  CHECK((16777215u < thr) == (draw(16777215u) < rate));
}
static void check_keep(float p, int32_t keep) {  // (k > keep) <=> (draw(k) > p)
  for (int d = -2; d <= 2; ++d) {
    const int64_t k = static_cast<int64_t>(keep) + d;
    if (k < 0 || k >= (1 << 24)) continue;
    CHECK((static_cast<int32_t>(k) > keep) == (draw(static_cast<uint32_t>(k)) > p));
  }
  CHECK((0 > keep) == (draw(0) > p));
  CHECK((16777215 > keep) == (draw(16777215u) > p));
}

static int expect_group(const bk_random_agents& r, uint32_t tick) {
  if (!(r.tick_lo < r.tick_hi) || !(r.vol_lo < r.vol_hi)) return BK_INVALID_ARGUMENT;
  if (r.tick_size % tick) return BK_PRICE_NOT_TICK_MULTIPLE;
  if (r.tick_lo == 0) return BK_INVALID_ARGUMENT;
  const unsigned __int128 top = static_cast<unsigned __int128>(r.tick_hi - 1) * r.tick_size;
  return top >= 0xFFFFFFFFull ? BK_INVALID_ARGUMENT : BK_OK;
}

static void one_group(const bk_random_agents& r, uint32_t tick) {
  Group a, b;
  std::memset(&a, 0xAB, sizeof(a));
  std::memset(&b, 0xCD, sizeof(b));
  uint32_t why = 99;
  const int sa = agent_rows::group_row(r, 0, tick, &a, &why);
  uint64_t total = 0;
  std::string msg;
  const int sb = make_groups(&r, 1, nullptr, 1, &tick, &b, &total, &msg);
  CHECK(sa == sb);
  CHECK(sa == expect_group(r, tick));
  CHECK((sa == BK_OK) == (why == agent_rows::WHY_NONE));
  CHECK((sa == BK_OK) == msg.empty());
  if (sa != BK_OK) return;
  CHECK(std::memcmp(&a, &b, sizeof(Group)) == 0);
  CHECK(a.n == r.n_agents && a.tick_lo == r.tick_lo && a.tick_rng == r.tick_hi - r.tick_lo && a.vol_lo == r.vol_lo &&
        a.vol_rng == r.vol_hi - r.vol_lo && a.tick_size == r.tick_size && a.asset == 0 && a.pad[0] == 0 && a.pad[1] == 0);
  // UniformInt<u32>::sample_single: zone = (range << range.leading_zeros()) - 1
  uint32_t lz = 0;
  while (!((a.tick_rng << lz) & 0x80000000u)) ++lz;
  CHECK(a.tick_zone == (a.tick_rng << lz) - 1u);
  check_rate(r.activity_rate, a.thr);
}

static int expect_member(const bk_agent_desc& m, uint32_t tick) {
  if (m.tick_size == 0 || m.tick_size % tick) return BK_PRICE_NOT_TICK_MULTIPLE;
  if (m.type == BK_AGENT_RANDOM) {
    if (!(m.tick_lo < m.tick_hi) || !(m.vol_lo < m.vol_hi) || m.tick_lo == 0) return BK_INVALID_ARGUMENT;
    return static_cast<unsigned __int128>(m.tick_hi - 1) * m.tick_size >= 0xFFFFFFFFull ? BK_INVALID_ARGUMENT : BK_OK;
  }
  if (m.type != BK_AGENT_NOISE && m.type != BK_AGENT_MOMENTUM) return BK_INVALID_ARGUMENT;
  if (m.n_agents > 65535u) return BK_INVALID_ARGUMENT;
  if (std::isnan(m.price_dist_sigma) || std::isinf(m.price_dist_sigma) || m.price_dist_sigma < 0.0) return BK_INVALID_ARGUMENT;
  if (std::isnan(m.price_dist_mu) || std::isinf(m.price_dist_mu)) return BK_INVALID_ARGUMENT;
  return BK_OK;
}

static void one_member(const bk_agent_desc& m, uint32_t tick, uint32_t slot_base) {
  // make_mixed_descs counts the fixed slots itself: a RandomAgents member of slot_base agents in front gives the same base
  bk_agent_desc pair[2];
  std::memset(pair, 0, sizeof(pair));
  pair[0].type = BK_AGENT_RANDOM, pair[0].n_agents = slot_base, pair[0].tick_lo = 1, pair[0].tick_hi = 2, pair[0].vol_lo = 1,
  pair[0].vol_hi = 2, pair[0].tick_size = tick;
  pair[1] = m;
  MixedDesc a, b[2];
  std::memset(&a, 0xAB, sizeof(a));
  std::memset(b, 0xCD, sizeof(b));
  uint32_t why = 99, fixed_a[MAX_ASSETS];
  const int sa = agent_rows::mixed_row(m, tick, slot_base, &a, &why);
  std::string msg;
  const int sb = make_mixed_descs(pair, 2, nullptr, &tick, b, fixed_a, &msg);
  CHECK(sa == sb);
  CHECK(sa == expect_member(m, tick));
  CHECK((sa == BK_OK) == (why == agent_rows::WHY_NONE));
  if (sa != BK_OK) return;
  CHECK(std::memcmp(&a, &b[1], sizeof(MixedDesc)) == 0);
  CHECK(a.type == m.type && a.n == m.n_agents && a.pad == 0);
  if (m.type == BK_AGENT_RANDOM) {
    CHECK(a.slot_base == slot_base && a.tick_size == m.tick_size && a.tick_rng == m.tick_hi - m.tick_lo);
    check_rate(m.activity_rate, a.thr);
  } else {
    check_rate(m.p_limit, a.thr_limit);
    check_rate(m.p_market, a.thr_market);
    check_keep(m.p_cancel, a.keep_thr);
    CHECK(a.mu == m.price_dist_mu && a.sigma == m.price_dist_sigma && a.decay == m.decay && a.demand == m.demand &&
          a.scale == m.scale && a.order_ratio == m.order_ratio && a.n_f == static_cast<double>(m.n_agents) &&
          a.tick_f == static_cast<double>(m.tick_size) && a.trade_vol == m.trade_vol && a.slot_base == 0);
  }
}

int main() {
  std::mt19937_64 rng(20240607);
  auto u = [&](uint32_t lo, uint32_t hi) { return lo + static_cast<uint32_t>(rng() % (hi - lo + 1)); };
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float eps = 1.0f / 16777216.0f;
  const std::vector<float> rates = {0.0f, 1.0f, nan, 1.5f, -0.25f, inf, -inf, eps, 2 * eps, 1.0f - eps, 1.0f - 2 * eps,
                                    std::nextafter(eps, 0.0f), std::nextafter(eps, 1.0f), 0.5f, std::nextafter(0.5f, 1.0f),
                                    std::nextafter(1.0f, 2.0f), 1e-30f, 0.3f};
  size_t n_rows = 0;

  // ---- groups: the edge rows, each with every rate
  const bk_random_agents good{64, 10, 20, 1, 5, 2, 0.5f};
  std::vector<bk_random_agents> edges = {good};
  auto edge = [&](auto f) {
    bk_random_agents r = good;
    f(r);
    edges.push_back(r);
  };
  edge([](bk_random_agents& r) { r.tick_hi = r.tick_lo; });             // empty tick range
  edge([](bk_random_agents& r) { r.tick_hi = r.tick_lo - 1; });
  edge([](bk_random_agents& r) { r.vol_hi = r.vol_lo; });               // empty vol range
  edge([](bk_random_agents& r) { r.tick_lo = 0; });                     // a price of 0
  edge([](bk_random_agents& r) { r.tick_size = 3; });                   // no multiple of the book's tick (2)
  edge([](bk_random_agents& r) { r.tick_size = 0; });                   // (0 is a multiple: every price is 0 ... and passes the bound)
  edge([](bk_random_agents& r) { r.tick_size = 1, r.tick_hi = 0xFFFFFFFFu; });   // top price u32::MAX - 1: one below the bound
  edge([](bk_random_agents& r) { r.tick_size = 1, r.tick_lo = 0xFFFFFFFEu, r.tick_hi = 0xFFFFFFFFu; });
  edge([](bk_random_agents& r) { r.tick_size = 2, r.tick_hi = 0x80000000u; });   // (2^31 - 1) * 2 = u32::MAX - 1: passes
  edge([](bk_random_agents& r) { r.tick_size = 0xFFFFFFFFu, r.tick_lo = 1, r.tick_hi = 3; });  // far beyond
  edge([](bk_random_agents& r) { r.vol_lo = 0, r.vol_hi = 0xFFFFFFFFu; });
  edge([](bk_random_agents& r) { r.n_agents = 0; });
  for (const bk_random_agents& e : edges)
    for (float rate : rates) {
      bk_random_agents r = e;
      r.activity_rate = rate;
      one_group(r, e.tick_size == 1 || e.tick_size == 0xFFFFFFFFu ? 1u : 2u);
      ++n_rows;
    }
  // exactly at the bound: (tick_hi - 1) * tick_size == u32::MAX is refused, one below is taken (tick 1 and a divisor pair)
  {
    bk_random_agents r = good;
    r.tick_size = 3, r.tick_lo = 1, r.tick_hi = 0x55555555u + 1u;  // 0x55555555 * 3 = u32::MAX
    one_group(r, 1);
    CHECK(expect_group(r, 1) == BK_INVALID_ARGUMENT);
    r.tick_hi -= 1;  // 0x55555554 * 3 = u32::MAX - 3
    one_group(r, 1);
    CHECK(expect_group(r, 1) == BK_OK);
    r.tick_size = 1, r.tick_hi = 0xFFFFFFFFu;
    CHECK(expect_group(r, 1) == BK_OK);
    n_rows += 2;
  }
  for (int i = 0; i < 4000; ++i) {
    bk_random_agents r;
    const uint32_t tick = u(1, 4);
    r.n_agents = u(0, 300);
    r.tick_lo = u(0, 6) ? u(1, 2000) : u(0, 1);
    r.tick_hi = u(0, 8) ? r.tick_lo + u(1, 5000) : u(0, r.tick_lo);
    r.vol_lo = u(0, 50);
    r.vol_hi = u(0, 8) ? r.vol_lo + u(1, 1000) : u(0, r.vol_lo);
    r.tick_size = u(0, 5) ? tick * u(1, 9) : u(0, 40);
    if (!u(0, 15)) r.tick_size = 0xFFFFFFFFu / (r.tick_hi > 1 ? r.tick_hi - 1 : 1) + u(0, 1);  // around the bound
    r.activity_rate = u(0, 9) ? static_cast<float>(rng() >> 40) * eps : rates[u(0, static_cast<uint32_t>(rates.size()) - 1)];
    one_group(r, tick);
    ++n_rows;
  }

  // ---- members
  bk_agent_desc noise;
  std::memset(&noise, 0, sizeof(noise));
  noise.type = BK_AGENT_NOISE, noise.n_agents = 40, noise.tick_size = 2, noise.agent_id_start = 7, noise.p_limit = 0.3f,
  noise.p_market = 0.1f, noise.p_cancel = 0.2f, noise.trade_vol = 10, noise.price_dist_mu = 1.5, noise.price_dist_sigma = 0.5;
  bk_agent_desc mom = noise;
  mom.type = BK_AGENT_MOMENTUM, mom.decay = 0.9, mom.demand = 2.0, mom.scale = 0.01, mom.order_ratio = 0.5;
  bk_agent_desc rnd;
  std::memset(&rnd, 0, sizeof(rnd));
  rnd.type = BK_AGENT_RANDOM, rnd.n_agents = 30, rnd.tick_lo = 10, rnd.tick_hi = 20, rnd.vol_lo = 1, rnd.vol_hi = 5,
  rnd.tick_size = 2, rnd.activity_rate = 0.5f;
  std::vector<bk_agent_desc> medges = {noise, mom, rnd};
  auto medge = [&](const bk_agent_desc& base, auto f) {
    bk_agent_desc m = base;
    f(m);
    medges.push_back(m);
  };
  const double dinf = std::numeric_limits<double>::infinity(), dnan = std::numeric_limits<double>::quiet_NaN();
  for (const bk_agent_desc& base : {noise, mom}) {
    medge(base, [&](bk_agent_desc& m) { m.price_dist_sigma = -0.5; });
    medge(base, [&](bk_agent_desc& m) { m.price_dist_sigma = -0.0; });
    medge(base, [&](bk_agent_desc& m) { m.price_dist_sigma = 0.0; });
    medge(base, [&](bk_agent_desc& m) { m.price_dist_sigma = dnan; });
    medge(base, [&](bk_agent_desc& m) { m.price_dist_sigma = dinf; });
    medge(base, [&](bk_agent_desc& m) { m.price_dist_mu = dnan; });
    medge(base, [&](bk_agent_desc& m) { m.price_dist_mu = -dinf; });
    medge(base, [&](bk_agent_desc& m) { m.n_agents = 65535; });
    medge(base, [&](bk_agent_desc& m) { m.n_agents = 65536; });
    medge(base, [&](bk_agent_desc& m) { m.tick_size = 0; });
    medge(base, [&](bk_agent_desc& m) { m.tick_size = 3; });
    medge(base, [&](bk_agent_desc& m) { m.type = 3; });
    medge(base, [&](bk_agent_desc& m) { m.type = 0xFFFFFFFFu; });
    for (float rate : rates) {
      medge(base, [&](bk_agent_desc& m) { m.p_limit = rate; });
      medge(base, [&](bk_agent_desc& m) { m.p_market = rate; });
      medge(base, [&](bk_agent_desc& m) { m.p_cancel = rate; });
    }
  }
  medge(rnd, [](bk_agent_desc& m) { m.tick_hi = m.tick_lo; });
  medge(rnd, [](bk_agent_desc& m) { m.vol_hi = m.vol_lo; });
  medge(rnd, [](bk_agent_desc& m) { m.tick_lo = 0; });
  medge(rnd, [](bk_agent_desc& m) { m.tick_size = 0; });
  medge(rnd, [](bk_agent_desc& m) { m.tick_size = 3; });
  medge(rnd, [](bk_agent_desc& m) { m.tick_size = 2, m.tick_hi = 0x80000000u; });       // one below the bound
  medge(rnd, [](bk_agent_desc& m) { m.tick_size = 2, m.tick_hi = 0x80000001u; });       // 2^32: beyond
  for (float rate : rates) medge(rnd, [&](bk_agent_desc& m) { m.activity_rate = rate; });
  for (const bk_agent_desc& m : medges) {
    one_member(m, 2, 0);
    one_member(m, 1, 17);
    n_rows += 2;
  }
  {  // exactly at the bound
    bk_agent_desc m = rnd;
    m.tick_size = 3, m.tick_lo = 1, m.tick_hi = 0x55555556u;
    one_member(m, 1, 5);
    CHECK(expect_member(m, 1) == BK_INVALID_ARGUMENT);
    m.tick_hi -= 1;
    one_member(m, 1, 5);
    CHECK(expect_member(m, 1) == BK_OK);
  }
  for (int i = 0; i < 4000; ++i) {
    bk_agent_desc m = u(0, 2) == 0 ? rnd : (u(0, 1) ? noise : mom);
    const uint32_t tick = u(1, 4);
    m.n_agents = u(0, 20) ? u(0, 300) : u(65530, 65540);
    m.tick_size = u(0, 5) ? tick * u(1, 9) : u(0, 40);
    m.tick_lo = u(0, 6) ? u(1, 2000) : u(0, 1);
    m.tick_hi = u(0, 8) ? m.tick_lo + u(1, 5000) : u(0, m.tick_lo);
    m.vol_hi = u(0, 8) ? m.vol_lo + u(1, 1000) : u(0, m.vol_lo);
    m.activity_rate = static_cast<float>(rng() >> 40) * eps;
    m.p_limit = u(0, 9) ? static_cast<float>(rng() >> 40) * eps : rates[u(0, static_cast<uint32_t>(rates.size()) - 1)];
    m.p_market = static_cast<float>(rng() >> 40) * eps;
    m.p_cancel = u(0, 9) ? static_cast<float>(rng() >> 40) * eps : rates[u(0, static_cast<uint32_t>(rates.size()) - 1)];
    m.price_dist_sigma = u(0, 12) ? static_cast<double>(rng() >> 11) * 1e-16 : (u(0, 1) ? -1.0 : dnan);
    m.price_dist_mu = u(0, 12) ? static_cast<double>(rng() >> 11) * 1e-15 - 4.0 : dinf;
    if (!u(0, 30)) m.type = u(3, 9);
    one_member(m, tick, u(0, 100));
    ++n_rows;
  }

  // ---- the retune's fixed fields
  {
    Group cur{}, next{};
    cur.n = next.n = 64;
    next.thr = 5, next.tick_size = 9, next.asset = 3;  // (anything else may differ)
    CHECK(agent_rows::group_fixed_ok(next, cur) == BK_OK);
    next.n = 65;
    CHECK(agent_rows::group_fixed_ok(next, cur) == BK_INVALID_ARGUMENT);
    MixedDesc c{}, n{};
    c.type = n.type = BK_AGENT_NOISE, c.n = n.n = 40;
    n.mu = 3.0, n.trade_vol = 9;
    CHECK(agent_rows::mixed_fixed_ok(n, c, 7, 7) == BK_OK);
    CHECK(agent_rows::mixed_fixed_ok(n, c, 8, 7) == BK_INVALID_ARGUMENT);
    n.n = 41;
    CHECK(agent_rows::mixed_fixed_ok(n, c, 7, 7) == BK_INVALID_ARGUMENT);
    n.n = 40, n.type = BK_AGENT_MOMENTUM;
    CHECK(agent_rows::mixed_fixed_ok(n, c, 7, 7) == BK_INVALID_ARGUMENT);
  }

  if (failures) {
    std::printf("agent_rows: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("agent_rows ok: %zu rows\n", n_rows);
  return 0;
}
