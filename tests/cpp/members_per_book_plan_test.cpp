// CPU test of the members' per-unit table in bourse_amd/csrc/pipeline_plan.hpp (run by tests/test_members_per_book_cpu.py):
// over the shapes of pipeline_plan_expected.txt (its first five columns: R n_books M agents request) and the settings grid
// of per_book_plan_test.cpp - explicit parts, fused_resident, warming, step_decode, order_log - a plan with
// PlanInput::members_per_book set
//   * has members_per_book exactly when the flag is set and AgentSet members are installed (n_mixed > 0);
//   * equals, field for field, the plan made without the table in every other field: every mixed kind has a PB form, so
//     kind, parts, stagger, priority and write_last stay.
#include <cstdio>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <tuple>

#include "../../bourse_amd/csrc/pipeline_plan.hpp"

using namespace bkd;

static int failures = 0;
#define CHECK(c, in)                                                                                                     \
  do {                                                                                                                   \
    if (!(c) && failures++ < 20)                                                                                         \
      std::printf("FAIL %s:%d: %s (R=%d books=%u M=%u groups=%d mixed=%u request=%d fr=%u warm=%d sd=%d log=%d)\n",    \
                  __FILE__, __LINE__, #c, (in).R, (in).n_books, (in).M, (in).groups, (in).n_mixed, (in).request,        \
                  (in).fused_resident, (in).warming, (in).step_decode, (in).order_log);                                 \
  } while (0)

static bool same(const Plan& a, const Plan& b) {
  return a.kind == b.kind && a.parts == b.parts && a.agents == b.agents && a.step_mkt == b.step_mkt &&
         a.step_poolpend == b.step_poolpend && a.stagger_us == b.stagger_us && a.step_prio == b.step_prio &&
         a.write_last == b.write_last && a.step_decode == b.step_decode && a.step_log == b.step_log &&
         a.agents_per_book == b.agents_per_book && a.members_per_book == b.members_per_book;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: members_per_book_plan_test <pipeline_plan_expected.txt>\n");
    return 2;
  }
  std::ifstream f(argv[1]);
  std::string line;
  std::set<std::tuple<int, uint32_t, uint32_t, int, int>> shapes;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream is(line);
    int R, agents, request;
    uint32_t n_books, M;
    if (is >> R >> n_books >> M >> agents >> request) shapes.emplace(R, n_books, M, agents, request);
  }
  size_t points = 0, per_book = 0;
  std::set<int> kinds;
  for (const auto& sh : shapes)
    for (int explicit_parts = 0; explicit_parts < 2; ++explicit_parts)
      for (uint32_t fr : {0u, 6144u, 4096u, 2048u})
        for (int warm = 0; warm < 2; ++warm)
          for (int sd = 0; sd < 2; ++sd)
            for (int log = 0; log < 2; ++log) {
              PlanInput in;
              in.R = std::get<0>(sh);
              in.n_books = std::get<1>(sh);
              in.M = std::get<2>(sh);
              in.groups = std::get<3>(sh) == 1;
              in.n_mixed = std::get<3>(sh) == 2 ? 2u : 0u;
              in.request = std::get<4>(sh);
              if (explicit_parts) in.n_parts = 3, in.min_part = 512, in.wave_parts = 3;
              in.fused_resident = fr;
              in.warming = warm;
              in.step_decode = sd;
              in.order_log = log;
              ++points;
              const Plan off = make_plan(in);
              CHECK(!in.members_per_book && !off.members_per_book, in);
              PlanInput pin = in;
              pin.members_per_book = true;
              const Plan on = make_plan(pin);
              CHECK(on.members_per_book == (in.n_mixed > 0), in);
              if (on.members_per_book) {
                ++per_book;
                kinds.insert(on.kind);
              }
              Plan want = off;
              want.members_per_book = on.members_per_book;
              CHECK(same(on, want), in);
            }
  if (shapes.size() != 4 * 17 * 3 * 3 * 6) {
    std::printf("FAIL: %zu shapes\n", shapes.size());
    ++failures;
  }
  // every mixed kind is reached with the table: k_run_mixed, the wave decode, the lane kernel, the wave-per-book kernel
  if (kinds != std::set<int>{PL_MIXED_FUSED, PL_MIXED_WAVE, PL_MIXED_LANES, PL_MIXED_WPB}) {
    std::printf("FAIL: the grid reaches %zu of the four mixed kinds with the table\n", kinds.size());
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("members_per_book_plan ok: %zu shapes, %zu points, %zu per book\n", shapes.size(), points, per_book);
  return 0;
}
