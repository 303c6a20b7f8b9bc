// CPU test of bourse_amd/csrc/pipeline_plan.hpp (run by tests/test_pipeline_plan.py): the rule's fixed points, then every
// field of make_plan over a grid of shapes and settings against pipeline_plan_expected.txt - a table made once from the rule
// as it stood before it moved into the header.
//
// Table line: R n_books M agents request, then 32 tokens (run-length: token*count) in the order
//   explicit parts {no, yes} x fused_resident {0, 6144, 4096, 2048} x warming {no, yes} x step_decode {no, yes};
// agents 0 none / 1 RandomAgents groups / 2 AgentSet members; explicit parts = set_split_parts(3, 512) + set_wave_options(64, 3).
// Token: kind parts agents step_mkt step_poolpend step_prio write_last step_decode "," stagger_us.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../bourse_amd/csrc/pipeline_plan.hpp"

using namespace bkd;

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static PlanInput shape(int R, uint32_t n_books, uint32_t M, int agents, int request) {
  PlanInput in;
  in.R = R;
  in.n_books = n_books;
  in.M = M;
  in.groups = agents == 1;
  in.n_mixed = agents == 2 ? 2u : 0u;
  in.request = request;
  return in;
}

static std::string token(const Plan& p) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%d%d%d%d%d%d%d%d,%u", static_cast<int>(p.kind), p.parts, static_cast<int>(p.agents), p.step_mkt,
                p.step_poolpend, p.step_prio, p.write_last, p.step_decode, p.stagger_us);
  return buf;
}

static void fixed_points() {
  // C3: 65 536 books, 128-slot pools -> the lane split in four parts, started 30 us apart
  PlanInput c3 = shape(2, 65536, 1, 1, 0);
  c3.fused_resident = 6144;
  Plan p = make_plan(c3);
  CHECK(p.kind == PL_SPLIT_LANES && p.parts == 4 && p.agents == AG_FSM && p.stagger_us == 30 && !p.step_prio);
  // the C3 shard of 8 192 books -> wave_split, four parts, the event waves at priority 1
  PlanInput shard = c3;
  shard.n_books = 8192;
  p = make_plan(shard);
  CHECK(p.kind == PL_SPLIT_WAVE && p.parts == 4 && p.agents == AG_WAVE && p.step_prio && p.stagger_us == 0);
  // C2: 4 096 books, 64-slot pools -> the persistent wave kernel
  PlanInput c2 = shape(1, 4096, 1, 1, 0);
  c2.fused_resident = 6144;
  CHECK(make_plan(c2).kind == PL_FUSED_WAVE);
  // markets -> the lane split (one lane per market), k_step_batch<R, MKT>
  p = make_plan(shape(1, 4096, 2, 1, 0));
  CHECK(p.kind == PL_SPLIT_LANES && p.agents == AG_FSM && p.step_mkt && !p.step_poolpend);
  p = make_plan(shape(1, 4096, 2, 2, 0));
  CHECK(p.kind == PL_MIXED_LANES && p.agents == AG_MIXED_LANES_MKT && p.step_mkt && p.step_poolpend && p.write_last);
  // AgentSet members from 512 books -> the wave-parallel members' update; below it the fused kernel
  p = make_plan(shape(8, 512, 1, 2, 0));
  CHECK(p.kind == PL_MIXED_WAVE && p.agents == AG_MIXED_WAVE && p.step_poolpend && p.write_last);
  CHECK(make_plan(shape(8, 511, 1, 2, 0)).kind == PL_MIXED_FUSED);
  // BOURSE_AMD_STAGGER_US overrides the default stagger; k_step_decode only on wave_split and never while warming
  c3.stagger_us = 0;
  CHECK(make_plan(c3).stagger_us == 0);
  shard.step_decode = true;
  CHECK(make_plan(shard).step_decode);
  shard.warming = true;
  CHECK(!make_plan(shard).step_decode);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: pipeline_plan_test <expected table>\n");
    return 2;
  }
  fixed_points();
  std::ifstream f(argv[1]);
  std::string line;
  size_t rows = 0, points = 0;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream is(line);
    int R, agents, request;
    uint32_t n_books, M;
    is >> R >> n_books >> M >> agents >> request;
    std::vector<std::string> want;
    std::string t;
    while (is >> t) {
      const size_t star = t.find('*');
      const int n = star == std::string::npos ? 1 : std::atoi(t.c_str() + star + 1);
      want.insert(want.end(), n, t.substr(0, star));
    }
    std::vector<std::string> got;
    for (int explicit_parts = 0; explicit_parts < 2; ++explicit_parts)
      for (uint32_t fr : {0u, 6144u, 4096u, 2048u})
        for (int warm = 0; warm < 2; ++warm)
          for (int sd = 0; sd < 2; ++sd) {
            PlanInput in = shape(R, n_books, M, agents, request);
            if (explicit_parts) in.n_parts = 3, in.min_part = 512, in.wave_parts = 3;
            in.fused_resident = fr;
            in.warming = warm;
            in.step_decode = sd;
            got.push_back(token(make_plan(in)));
          }
    if (got.size() != want.size()) {
      std::printf("FAIL row %zu: %zu tokens, expected %zu\n", rows, want.size(), got.size());
      ++failures;
    }
    for (size_t i = 0; i < got.size() && i < want.size(); ++i, ++points)
      if (got[i] != want[i] && failures++ < 20)
        std::printf("FAIL R=%d books=%u M=%u agents=%d request=%d point %zu: %s, expected %s\n", R, n_books, M, agents, request, i,
                    got[i].c_str(), want[i].c_str());
    ++rows;
  }
  if (rows != 4 * 17 * 3 * 3 * 6) {
    std::printf("FAIL: %zu table rows\n", rows);
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("pipeline_plan ok: %zu rows, %zu points\n", rows, points);
  return 0;
}
