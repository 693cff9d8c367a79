// isle_amd/host/plan_bound_main.cpp — plan_bound of ../csrc/stage_host.h, the rule behind isle_hip_plan_shards and the plan of the tdf
// counting stream, without the library and without a GPU (tests/test_tdf_shard_rule_cpu.py builds it with the address and
// undefined-behaviour sanitizers).  stdin, one plan per line: "<parts> <D> <weight of document 0> ... <weight of document D - 1>";
// stdout: the parts + 1 bounds of each, on one line.  The offsets are the running sums of the weights, as the device's scan forms them.
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/stage_host.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    long long parts = 0, D = -1;
    if (!(in >> parts >> D) || parts < 1 || D < 0) {
      std::cerr << "plan_bound_main: bad line: " << line << "\n";
      return 2;
    }
    std::vector<int64_t> offs((size_t)D + 1, 0);
    for (long long d = 0; d < D; ++d) {
      long long w = 0;
      if (!(in >> w) || w < 0) {
        std::cerr << "plan_bound_main: bad weight in: " << line << "\n";
        return 2;
      }
      offs[(size_t)d + 1] = offs[(size_t)d] + w;
    }
    std::vector<uint64_t> bounds((size_t)parts + 1, 0);
    for (int p = 1; p < (int)parts; ++p) bounds[(size_t)p] = plan_bound(offs.data(), (uint64_t)D, p, (int)parts, bounds[(size_t)p - 1]);
    bounds[(size_t)parts] = (uint64_t)D;
    for (size_t p = 0; p < bounds.size(); ++p) std::cout << (p ? " " : "") << bounds[p];
    std::cout << "\n";
  }
  return 0;
}
