// CPU test of the per-unit parameter table's rule in bourse_amd/csrc/pipeline_plan.hpp (run by tests/test_per_book_plan.py):
// over the shapes of pipeline_plan_expected.txt (its first five columns: R n_books M agents request) and the same settings
// grid - explicit parts, fused_resident, warming, step_decode, order_log - a plan with PlanInput::per_book set
//   * has agents_per_book exactly when RandomAgents groups are installed without Noise / Momentum members;
//   * never runs k_run_random then: the "fused" request on RandomAgents books takes the lane split (k_run_wave, wave_split
//     and split keep their choice and run their PB forms);
//   * has step_decode off whenever agents_per_book is on;
//   * equals, field for field, the plan made without the table (of the split kind it maps to) in every other field.
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
         a.agents_per_book == b.agents_per_book;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: per_book_plan_test <pipeline_plan_expected.txt>\n");
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
  size_t points = 0, per_book = 0, remapped = 0, fused_wave = 0;
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
              // per_book off (the default): no PB kernel anywhere
              const Plan off = make_plan(in);
              CHECK(!in.per_book, in);
              CHECK(!off.agents_per_book, in);
              PlanInput pin = in;
              pin.per_book = true;
              const Plan on = make_plan(pin);
              CHECK(on.agents_per_book == (in.groups && !in.n_mixed), in);
              CHECK(!(on.agents_per_book && on.step_decode), in);
              if (on.agents_per_book) CHECK(on.kind != PL_FUSED_RANDOM, in);
              per_book += on.agents_per_book;
              fused_wave += on.agents_per_book && on.kind == PL_FUSED_WAVE;
              // every other field: the plan of the kind it runs, made without the table
              PlanInput ref = in;
              if (on.kind != off.kind) {
                ++remapped;
                CHECK(off.kind == PL_FUSED_RANDOM && on.kind == PL_SPLIT_LANES && in.groups && !in.n_mixed, in);
                CHECK(in.request == 1, in);  // (auto never picks k_run_random for RandomAgents books)
                ref.request = 2;
              }
              Plan want = make_plan(ref);
              CHECK(want.kind == on.kind, in);
              want.agents_per_book = on.agents_per_book;
              if (on.agents_per_book) want.step_decode = false;
              CHECK(same(on, want), in);
            }
  if (shapes.size() != 4 * 17 * 3 * 3 * 6) {
    std::printf("FAIL: %zu shapes\n", shapes.size());
    ++failures;
  }
  if (!remapped || !fused_wave) {
    std::printf("FAIL: the grid has no remapped (%zu) or per-book k_run_wave (%zu) point\n", remapped, fused_wave);
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("per_book_plan ok: %zu shapes, %zu points, %zu per book, %zu remapped\n", shapes.size(), points, per_book,
              remapped);
  return 0;
}
