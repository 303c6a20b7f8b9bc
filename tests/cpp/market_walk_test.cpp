// market_walk_test.cpp - bourse_amd/csrc/market_walk.hpp on the CPU (tests/test_market_ingress_cpu.py).
// usage: market_walk_test <lists.txt> <passes.txt>
//   lists.txt:  the number of lists, then per list "n_groups" and n_groups pairs "n asset"
//   passes.txt: per list one line "first len asset trader0 group" per pass, then a line "-"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/market_walk.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  unsigned n_lists = 0;
  if (std::fscanf(in, "%u", &n_lists) != 1) return 2;
  for (unsigned i = 0; i < n_lists; ++i) {
    unsigned n_groups = 0;
    if (std::fscanf(in, "%u", &n_groups) != 1) return 2;
    std::vector<uint32_t> n(n_groups), asset(n_groups);
    for (unsigned g = 0; g < n_groups; ++g)
      if (std::fscanf(in, "%u %u", &n[g], &asset[g]) != 2) return 2;
    bkd::ingress::PassCursor c;
    bkd::ingress::MarketPass p;
    while (bkd::ingress::next_pass(
        c, n_groups, [&](uint32_t g) { return n[g]; }, [&](uint32_t g) { return asset[g]; }, p))
      std::fprintf(out, "%u %u %u %u %u\n", p.first, p.len, p.asset, p.trader0, p.group);
    std::fprintf(out, "-\n");
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("market_walk ok %u lists\n", n_lists);
  return 0;
}
