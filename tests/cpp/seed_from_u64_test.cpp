// bourse_amd/csrc/host_math.hpp seed_from_u64 compiled for the host: the SAME text hipcc compiles for the device
// (book_reset.hpp re-seeds reset books with it).  Prints "seed s0 s1" for every seed on the command line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../bourse_amd/csrc/host_math.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const uint64_t seed = std::strtoull(argv[i], nullptr, 10);
    uint64_t s0 = 0, s1 = 0;
    bkd::seed_from_u64(seed, s0, s1);
    std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", seed, s0, s1);
  }
  return 0;
}
