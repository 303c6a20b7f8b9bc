// CPU test of the host builder of bk_set_random_agents_per_book's table (bourse_amd/csrc/agent_table.hpp; run by
// tests/test_per_book_table_cpu.py):
//   * a unit's records are exactly what the uniform call (bk_set_random_market_agents -> make_groups) builds from that row,
//     and make_groups' records follow activity_threshold / sample_zone field by field;
//   * every status code of the uniform call, with the failing unit and group named in the message; the uniform call's
//     messages carry no prefix;
//   * n_agents differing between units is refused; capacity is checked per unit;
//   * on a failure the output table is left as it was;
//   * the hash is equal for equal tables and differs otherwise.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../bourse_amd/csrc/agent_table.hpp"

using namespace bkd;

static int failures = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c) && failures++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
  } while (0)

static bool same_records(const Group* a, const Group* b, size_t n) { return std::memcmp(a, b, n * sizeof(Group)) == 0; }

int main() {
  const uint32_t M = 1, tick[8] = {2, 2, 2, 2, 2, 2, 2, 2};
  const uint32_t U = 37, G = 3;
  std::mt19937 gen(7);
  auto rnd = [&](uint32_t lo, uint32_t hi) { return lo + gen() % (hi - lo + 1); };
  std::vector<bk_random_agents> rows(U * G);
  const uint32_t n_agents[G] = {64, 37, 91};
  for (uint32_t u = 0; u < U; ++u)
    for (uint32_t g = 0; g < G; ++g) {
      bk_random_agents& r = rows[u * G + g];
      r.n_agents = n_agents[g];
      r.tick_lo = rnd(1, 500);
      r.tick_hi = r.tick_lo + (u % 5 == 0 ? 1 : rnd(1, 4000));  // (ranges of width 1 and wide ones)
      r.vol_lo = rnd(1, 50);
      r.vol_hi = r.vol_lo + (u % 7 == 0 ? 1 : rnd(1, 100));
      r.tick_size = 2 * rnd(1, 4);
      const float rates[4] = {0.0f, 1.0f, 0.3f, 0.77f};
      r.activity_rate = rates[(u + g) % 4];
    }
  // ---- a row's records = the uniform call's preprocessing of that row
  std::vector<Group> t;
  uint64_t total = 0;
  std::string msg;
  CHECK(make_group_table(rows.data(), U, G, nullptr, M, tick, 192, t, &total, &msg) == BK_OK);
  CHECK(t.size() == U * G && total == 64 + 37 + 91);
  for (uint32_t u = 0; u < U; ++u) {
    Group one[G];
    uint64_t tot = 0;
    CHECK(make_groups(rows.data() + u * G, G, nullptr, M, tick, one, &tot, &msg) == BK_OK);
    CHECK(same_records(one, t.data() + u * G, G));
    for (uint32_t g = 0; g < G; ++g) {
      const bk_random_agents& r = rows[u * G + g];
      const Group& x = t[u * G + g];
      CHECK(x.n == r.n_agents && x.thr == activity_threshold(r.activity_rate));
      CHECK(x.tick_lo == r.tick_lo && x.tick_rng == r.tick_hi - r.tick_lo && x.tick_zone == sample_zone(x.tick_rng));
      CHECK(x.vol_lo == r.vol_lo && x.vol_rng == r.vol_hi - r.vol_lo && x.vol_zone == sample_zone(x.vol_rng));
      CHECK(x.tick_size == r.tick_size && x.asset == 0 && x.pad[0] == 0 && x.pad[1] == 0);
    }
  }
  CHECK(activity_threshold(0.0f) == 0u && activity_threshold(1.0f) == 1u << 24);
  // ---- refusals: the code of the uniform call, the unit and group named; the table untouched
  const std::vector<Group> keep = t;
  struct Bad {
    uint32_t u, g;
    int code;
    const char* what;
    void (*apply)(bk_random_agents&);
  };
  const Bad bad[] = {
      {5, 1, BK_INVALID_ARGUMENT, "empty tick/vol range", [](bk_random_agents& r) { r.tick_hi = r.tick_lo; }},
      {9, 2, BK_INVALID_ARGUMENT, "empty tick/vol range", [](bk_random_agents& r) { r.vol_hi = r.vol_lo - 1; }},
      {11, 0, BK_PRICE_NOT_TICK_MULTIPLE, "agent tick_size must be a multiple of the env tick_size",
       [](bk_random_agents& r) { r.tick_size = 3; }},
      {17, 1, BK_INVALID_ARGUMENT, "limit prices must lie in (0, u32::MAX)", [](bk_random_agents& r) { r.tick_lo = 0; }},
      {36, 2, BK_INVALID_ARGUMENT, "limit prices must lie in (0, u32::MAX)",
       [](bk_random_agents& r) { r.tick_hi = 0x7FFFFFFFu, r.tick_size = 4; }},
      {3, 1, BK_INVALID_ARGUMENT, "n_agents differs from unit 0's", [](bk_random_agents& r) { r.n_agents += 1; }},
  };
  for (const Bad& b : bad) {
    std::vector<bk_random_agents> rr = rows;
    b.apply(rr[b.u * G + b.g]);
    std::vector<bk_random_agents> later = rr;  // (a later unit fails too: the FIRST failing one is named)
    if (b.u + 1 < U) later[(U - 1) * G].tick_hi = later[(U - 1) * G].tick_lo;
    for (const auto* src : {&rr, &later}) {
      std::vector<Group> out = keep;
      msg.clear();
      const int rc = make_group_table(src->data(), U, G, nullptr, M, tick, 192, out, &total, &msg);
      const std::string where = "unit " + std::to_string(b.u) + ", group " + std::to_string(b.g) + ": ";
      CHECK(rc == b.code);
      CHECK(msg.rfind(where, 0) == 0 && msg.find(b.what) != std::string::npos);
      if (msg.rfind(where, 0) != 0) std::printf("  message: %s\n", msg.c_str());
      CHECK(same_records(out.data(), keep.data(), keep.size()) && out.size() == keep.size());
    }
    if (b.code != BK_INVALID_ARGUMENT || std::string(b.what).find("n_agents") == std::string::npos) {
      Group one[G];
      uint64_t tot = 0;
      std::string m1;
      CHECK(make_groups(rr.data() + b.u * G, G, nullptr, M, tick, one, &tot, &m1) == b.code);
      CHECK(m1 == b.what);  // the uniform call's message, as before
    }
  }
  {  // asset out of range (markets): the uniform call's code
    const uint32_t assets[G] = {0, 2, 1};
    std::vector<Group> out;
    CHECK(make_group_table(rows.data(), U, G, assets, 2, tick, 192, out, &total, &msg) == BK_INVALID_ARGUMENT);
    CHECK(msg == "unit 0, group 1: group asset index out of range");
    const uint32_t ok_assets[G] = {0, 1, 1};
    CHECK(make_group_table(rows.data(), U, G, ok_assets, 2, tick, 192, out, &total, &msg) == BK_OK);
    CHECK(out[G + 1].asset == 1 && out[G + 2].asset == 1 && out[G].asset == 0);
  }
  {  // capacity: a unit's agents must fit max_live_orders
    std::vector<Group> out = keep;
    CHECK(make_group_table(rows.data(), U, G, nullptr, M, tick, 191, out, &total, &msg) == BK_CAPACITY);
    CHECK(msg == std::string("unit 0, ") + CAPACITY_MSG);
    CHECK(same_records(out.data(), keep.data(), keep.size()));
  }
  // ---- the hash: equal tables hash equal, any change of a record changes it
  {
    std::vector<Group> t2;
    CHECK(make_group_table(rows.data(), U, G, nullptr, M, tick, 192, t2, &total, &msg) == BK_OK);
    CHECK(groups_hash(t.data(), t.size()) == groups_hash(t2.data(), t2.size()));
    std::vector<bk_random_agents> rr = rows;
    rr[20 * G + 2].activity_rate = std::nextafter(rr[20 * G + 2].activity_rate, 2.0f);
    rr[20 * G + 2].activity_rate = rr[20 * G + 2].activity_rate == 0.0f ? 0.5f : rr[20 * G + 2].activity_rate;
    CHECK(make_group_table(rr.data(), U, G, nullptr, M, tick, 192, t2, &total, &msg) == BK_OK);
    CHECK(groups_hash(t.data(), t.size()) != groups_hash(t2.data(), t2.size()));
    rr = rows;
    std::swap(rr[0], rr[G]);  // (two units' rows swapped: the same records, another table)
    std::swap(rr[1], rr[G + 1]);
    std::swap(rr[2], rr[G + 2]);
    CHECK(make_group_table(rr.data(), U, G, nullptr, M, tick, 192, t2, &total, &msg) == BK_OK);
    CHECK(groups_hash(t.data(), t.size()) != groups_hash(t2.data(), t2.size()));
    // identical rows of one unit's groups: the table's hash is not the uniform set's (another length)
    CHECK(groups_hash(t.data(), G) != groups_hash(t.data(), t.size()));
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("per_book_table ok: %u units x %u groups\n", U, G);
  return 0;
}
