// CPU test of the host builder of bk_set_agents_per_book's table (bourse_amd/csrc/agent_table.hpp; run by
// tests/test_members_per_book_cpu.py):
//   * a unit's records are exactly what the uniform call (set_agents_impl -> make_mixed_descs) builds from that row, and
//     make_mixed_descs' records follow the thresholds, zones and f64 fields member by member;
//   * every status code of the uniform call, with the failing unit and member named in the message; the uniform call's
//     messages carry no prefix;
//   * type or n_agents differing between units is refused; capacity is checked on the shared fixed slots;
//   * on a failure the output table is left as it was;
//   * the hash is equal for equal tables and differs otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../bourse_amd/csrc/agent_table.hpp"

using namespace bkd;

static int failures = 0;
#define CHECK(c)                                                                          \
  do {                                                                                    \
    if (!(c) && failures++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
  } while (0)

static bool same_records(const MixedDesc* a, const MixedDesc* b, size_t n) {
  return std::memcmp(a, b, n * sizeof(MixedDesc)) == 0;
}

int main() {
  const uint32_t M = 1, tick[8] = {2, 2, 2, 2, 2, 2, 2, 2};
  const uint32_t U = 29, N = 4;
  const uint32_t types[N] = {BK_AGENT_RANDOM, BK_AGENT_NOISE, BK_AGENT_MOMENTUM, BK_AGENT_NOISE};
  const uint32_t n_agents[N] = {40, 30, 25, 10};
  std::mt19937 gen(11);
  auto rnd = [&](uint32_t lo, uint32_t hi) { return lo + gen() % (hi - lo + 1); };
  auto unif = [&]() { return (gen() % 1000001) / 1000000.0; };
  std::vector<bk_agent_desc> rows(U * N);
  for (uint32_t u = 0; u < U; ++u)
    for (uint32_t i = 0; i < N; ++i) {
      bk_agent_desc& d = rows[u * N + i];
      std::memset(&d, 0, sizeof(d));
      d.type = types[i];
      d.n_agents = n_agents[i];
      d.tick_size = 2 * rnd(1, 4);
      if (d.type == BK_AGENT_RANDOM) {
        d.tick_lo = rnd(1, 500);
        d.tick_hi = d.tick_lo + rnd(1, 4000);
        d.vol_lo = rnd(1, 50);
        d.vol_hi = d.vol_lo + rnd(1, 100);
        d.activity_rate = static_cast<float>(unif());
      } else {
        const float ps[4] = {0.0f, 1.0f, 0.3f, 0.77f};
        d.agent_id_start = 100 * i;
        d.p_limit = ps[(u + i) % 4];
        d.p_market = ps[(u + 2 * i) % 4];
        d.p_cancel = static_cast<float>(unif());
        d.trade_vol = rnd(1, 200);
        d.price_dist_mu = unif() - 0.5;
        d.price_dist_sigma = u % 5 == 0 ? 0.0 : 3.0 * unif();
        d.decay = unif();
        d.demand = 10.0 * unif();
        d.scale = unif();
        d.order_ratio = 2.0 * unif();
      }
    }
  // ---- a row's records = the uniform call's preprocessing of that row
  std::vector<MixedDesc> t;
  uint32_t fixed_a[MAX_ASSETS];
  std::string msg;
  CHECK(make_mixed_table(rows.data(), U, N, nullptr, M, tick, 128, t, fixed_a, &msg) == BK_OK);
  CHECK(t.size() == U * N && fixed_a[0] == 40 && fixed_a[1] == 0);
  for (uint32_t u = 0; u < U; ++u) {
    MixedDesc one[N];
    uint32_t fa[MAX_ASSETS];
    CHECK(make_mixed_descs(rows.data() + u * N, N, nullptr, tick, one, fa, &msg) == BK_OK);
    CHECK(same_records(one, t.data() + u * N, N));
    CHECK(fa[0] == fixed_a[0]);
    for (uint32_t i = 0; i < N; ++i) {
      const bk_agent_desc& d = rows[u * N + i];
      const MixedDesc& x = t[u * N + i];
      CHECK(x.type == d.type && x.n == d.n_agents && x.pad == 0);
      if (d.type == BK_AGENT_RANDOM) {
        CHECK(x.thr == activity_threshold(d.activity_rate) && x.slot_base == 0 && x.tick_size == d.tick_size);
        CHECK(x.tick_lo == d.tick_lo && x.tick_rng == d.tick_hi - d.tick_lo && x.tick_zone == sample_zone(x.tick_rng));
        CHECK(x.vol_lo == d.vol_lo && x.vol_rng == d.vol_hi - d.vol_lo && x.vol_zone == sample_zone(x.vol_rng));
        CHECK(x.thr_limit == 0 && x.keep_thr == 0 && x.tick_f == 0.0);
      } else {
        CHECK(x.thr_limit == activity_threshold(d.p_limit) && x.thr_market == activity_threshold(d.p_market));
        CHECK(x.keep_thr == keep_threshold(d.p_cancel) && x.trade_vol == d.trade_vol);
        CHECK(x.mu == d.price_dist_mu && x.sigma == d.price_dist_sigma && x.decay == d.decay && x.demand == d.demand);
        CHECK(x.scale == d.scale && x.order_ratio == d.order_ratio);
        CHECK(x.n_f == static_cast<double>(d.n_agents) && x.tick_f == static_cast<double>(d.tick_size));
        CHECK(x.thr == 0 && x.tick_lo == 0 && x.slot_base == 0);
      }
    }
  }
  // ---- refusals: the code of the uniform call, the unit and member named; the table untouched
  const std::vector<MixedDesc> keep = t;
  struct Bad {
    uint32_t u, i;
    int code;
    const char* what;
    void (*apply)(bk_agent_desc&);
  };
  const Bad bad[] = {
      {5, 0, BK_INVALID_ARGUMENT, "bad RandomAgents ranges", [](bk_agent_desc& d) { d.tick_hi = d.tick_lo; }},
      {6, 0, BK_INVALID_ARGUMENT, "bad RandomAgents ranges", [](bk_agent_desc& d) { d.tick_lo = 0; }},
      {9, 1, BK_PRICE_NOT_TICK_MULTIPLE, "member tick_size must be a non-zero multiple of the env tick_size",
       [](bk_agent_desc& d) { d.tick_size = 3; }},
      {10, 2, BK_PRICE_NOT_TICK_MULTIPLE, "member tick_size must be a non-zero multiple of the env tick_size",
       [](bk_agent_desc& d) { d.tick_size = 0; }},
      {17, 2, BK_INVALID_ARGUMENT, "LogNormal::new(mu, sigma) needs finite mu and sigma >= 0",
       [](bk_agent_desc& d) { d.price_dist_sigma = -1.0; }},
      {18, 3, BK_INVALID_ARGUMENT, "LogNormal::new(mu, sigma) needs finite mu and sigma >= 0",
       [](bk_agent_desc& d) { d.price_dist_mu = std::nan(""); }},
      {28, 1, BK_INVALID_ARGUMENT, "unknown agent type", [](bk_agent_desc& d) { d.type = 7; }},
      {3, 1, BK_INVALID_ARGUMENT, "n_agents differs from unit 0's", [](bk_agent_desc& d) { d.n_agents += 1; }},
      {4, 3, BK_INVALID_ARGUMENT, "type differs from unit 0's", [](bk_agent_desc& d) { d.type = BK_AGENT_MOMENTUM; }},
      {7, 0, BK_INVALID_ARGUMENT, "n_agents differs from unit 0's", [](bk_agent_desc& d) { d.n_agents = 41; }},
  };
  for (const Bad& b : bad) {
    std::vector<bk_agent_desc> rr = rows;
    b.apply(rr[b.u * N + b.i]);
    std::vector<bk_agent_desc> later = rr;  // (a later unit fails too: the FIRST failing one is named)
    if (b.u + 1 < U) later[(U - 1) * N + 1].price_dist_sigma = -2.0;
    for (const auto* src : {&rr, &later}) {
      std::vector<MixedDesc> out = keep;
      msg.clear();
      const int rc = make_mixed_table(src->data(), U, N, nullptr, M, tick, 128, out, fixed_a, &msg);
      const std::string where = "unit " + std::to_string(b.u) + ", member " + std::to_string(b.i) + ": ";
      CHECK(rc == b.code);
      CHECK(msg.rfind(where, 0) == 0 && msg.find(b.what) != std::string::npos);
      if (msg.rfind(where, 0) != 0 || msg.find(b.what) == std::string::npos) std::printf("  message: %s\n", msg.c_str());
      CHECK(same_records(out.data(), keep.data(), keep.size()) && out.size() == keep.size());
    }
    if (std::string(b.what).find("differs") == std::string::npos) {
      MixedDesc one[N];
      uint32_t fa[MAX_ASSETS];
      std::string m1;
      CHECK(make_mixed_descs(rr.data() + b.u * N, N, nullptr, tick, one, fa, &m1) == b.code);
      CHECK(m1 == b.what);  // the uniform call's message, as before
    }
  }
  {  // markets: fixed slots per asset, tick sizes of the member's asset
    const uint32_t assets[N] = {1, 0, 1, 0}, mtick[8] = {2, 4, 1, 1, 1, 1, 1, 1};
    std::vector<MixedDesc> out;
    std::vector<bk_agent_desc> rr = rows;
    for (uint32_t u = 0; u < U; ++u) rr[u * N + 2].tick_size = 4 * (1 + u % 3), rr[u * N].tick_size = 8;
    CHECK(make_mixed_table(rr.data(), U, N, assets, 2, mtick, 128, out, fixed_a, &msg) == BK_OK);
    CHECK(fixed_a[0] == 0 && fixed_a[1] == 40);
    rr[3 * N + 2].tick_size = 6;  // (a multiple of asset 0's tick, not of asset 1's)
    CHECK(make_mixed_table(rr.data(), U, N, assets, 2, mtick, 128, out, fixed_a, &msg) == BK_PRICE_NOT_TICK_MULTIPLE);
    CHECK(msg.rfind("unit 3, member 2: ", 0) == 0);
  }
  {  // capacity: the RandomAgents members' fixed slots must leave room in max_live_orders
    std::vector<MixedDesc> out = keep;
    CHECK(make_mixed_table(rows.data(), U, N, nullptr, M, tick, 40, out, fixed_a, &msg) == BK_CAPACITY);
    CHECK(msg == std::string("unit 0, ") + MIXED_CAPACITY_MSG);
    CHECK(same_records(out.data(), keep.data(), keep.size()));
    CHECK(make_mixed_table(rows.data(), U, N, nullptr, M, tick, 41, out, fixed_a, &msg) == BK_OK);
  }
  // ---- the hash: equal tables hash equal, any change of a record changes it
  {
    const uint32_t member_asset[MAX_MEMBERS] = {0, 0, 0, 0};
    std::vector<MixedDesc> t2;
    CHECK(make_mixed_table(rows.data(), U, N, nullptr, M, tick, 128, t2, fixed_a, &msg) == BK_OK);
    CHECK(mixed_hash(member_asset, t.data(), t.size()) == mixed_hash(member_asset, t2.data(), t2.size()));
    std::vector<bk_agent_desc> rr = rows;
    rr[20 * N + 2].scale = std::nextafter(rr[20 * N + 2].scale, 2.0);
    CHECK(make_mixed_table(rr.data(), U, N, nullptr, M, tick, 128, t2, fixed_a, &msg) == BK_OK);
    CHECK(mixed_hash(member_asset, t.data(), t.size()) != mixed_hash(member_asset, t2.data(), t2.size()));
    rr = rows;
    for (uint32_t i = 0; i < N; ++i) std::swap(rr[i], rr[N + i]);  // (two units' rows swapped: the same records, another table)
    CHECK(make_mixed_table(rr.data(), U, N, nullptr, M, tick, 128, t2, fixed_a, &msg) == BK_OK);
    CHECK(mixed_hash(member_asset, t.data(), t.size()) != mixed_hash(member_asset, t2.data(), t2.size()));
    const uint32_t other_asset[MAX_MEMBERS] = {0, 1, 0, 0};
    CHECK(mixed_hash(member_asset, t.data(), t.size()) != mixed_hash(other_asset, t.data(), t.size()));
    // the uniform set of one row is not the table (another length)
    CHECK(mixed_hash(member_asset, t.data(), N) != mixed_hash(member_asset, t.data(), t.size()));
    // the uniform call's hash as before: FNV-1a of the records continued over the members' assets
    uint64_t h = 1469598103934665603ull;
    const unsigned char* c = reinterpret_cast<const unsigned char*>(t.data());
    for (size_t k = 0; k < N * sizeof(MixedDesc); ++k) h = (h ^ c[k]) * 1099511628211ull;
    c = reinterpret_cast<const unsigned char*>(member_asset);
    for (size_t k = 0; k < sizeof(member_asset); ++k) h = (h ^ c[k]) * 1099511628211ull;
    CHECK(mixed_hash(member_asset, t.data(), N) == h);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("members_per_book_table ok: %u units x %u members\n", U, N);
  return 0;
}
