// CPU test of the order-log rule of bourse_amd/csrc/pipeline_plan.hpp (run by tests/test_agent_order_log_plan.py): over the
// shapes of pipeline_plan_expected.txt (its first five columns: R n_books M agents request) and the same settings grid -
// explicit parts, fused_resident, warming, step_decode - a plan with PlanInput::order_log set
//   * is never a fused kind when RandomAgents groups are installed (the log is written by the split forms' event kernel);
//   * has step_log exactly when its kind is a split kind and the steps are not bk_warm's scratch steps;
//   * has step_decode off whenever step_log is on;
//   * equals, field for field, the plan of the split kind it maps to, run without the log;
// and the log is off by default (PlanInput{}.order_log) with no step_log in any plan without it.  What make_plan returns
// without the log is pinned by tests/test_pipeline_plan.py's table, whose inputs leave order_log at that default.
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
      std::printf("FAIL %s:%d: %s (R=%d books=%u M=%u groups=%d mixed=%u request=%d fr=%u warm=%d sd=%d)\n", __FILE__, \
                  __LINE__, #c, (in).R, (in).n_books, (in).M, (in).groups, (in).n_mixed, (in).request,                 \
                  (in).fused_resident, (in).warming, (in).step_decode);                                                  \
  } while (0)

static bool same(const Plan& a, const Plan& b) {
  return a.kind == b.kind && a.parts == b.parts && a.agents == b.agents && a.step_mkt == b.step_mkt &&
         a.step_poolpend == b.step_poolpend && a.stagger_us == b.stagger_us && a.step_prio == b.step_prio &&
         a.write_last == b.write_last && a.step_decode == b.step_decode && a.step_log == b.step_log;
}

// the request that makes the rule pick `kind` for this shape without the log (the split kinds of RandomAgents books)
static int request_of(PlanKind kind) { return kind == PL_SPLIT_WAVE ? 4 : 2; }

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: agent_order_log_plan_test <pipeline_plan_expected.txt>\n");
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
  size_t points = 0, logged = 0, remapped = 0;
  for (const auto& sh : shapes)
    for (int explicit_parts = 0; explicit_parts < 2; ++explicit_parts)
      for (uint32_t fr : {0u, 6144u, 4096u, 2048u})
        for (int warm = 0; warm < 2; ++warm)
          for (int sd = 0; sd < 2; ++sd) {
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
            ++points;
            // order_log off (the default): no logging kernel
            const Plan off = make_plan(in);
            CHECK(!in.order_log, in);
            CHECK(!off.step_log, in);
            // order_log = true
            PlanInput lin = in;
            lin.order_log = true;
            const Plan on = make_plan(lin);
            if (in.groups && !in.n_mixed) CHECK(is_split(on.kind), in);
            CHECK(on.step_log == (is_split(on.kind) && !in.warming), in);
            CHECK(!(on.step_log && on.step_decode), in);
            logged += on.step_log;
            // every other field: the plan of the split kind it runs, asked for without the log
            PlanInput ref = in;
            if (on.kind != off.kind) {
              ++remapped;
              CHECK((off.kind == PL_FUSED_WAVE && on.kind == PL_SPLIT_WAVE) ||
                        (off.kind == PL_FUSED_RANDOM && on.kind == PL_SPLIT_LANES),
                    in);
              ref.request = request_of(on.kind);
            }
            Plan want = make_plan(ref);
            CHECK(want.kind == on.kind, in);
            want.step_log = on.step_log;
            if (on.step_log) want.step_decode = false;
            CHECK(same(on, want), in);
          }
  if (shapes.size() != 4 * 17 * 3 * 3 * 6) {
    std::printf("FAIL: %zu shapes\n", shapes.size());
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("agent_order_log_plan ok: %zu shapes, %zu points, %zu logged, %zu remapped\n", shapes.size(), points, logged,
              remapped);
  return 0;
}
