// isle_amd/host/topic_sums_slice_main.cpp — topic_sums_slice of ../csrc/stage_host.h, the rule that cuts the L lines of
// DocTopicCatchwordSums.tsv among W ranks, and route_topic_sums of ../csrc/route_host.h, without the library and without a GPU
// (tests/test_doc_shard_cases_cpu.py builds it with the address and undefined-behaviour sanitizers).  stdin, one question per line:
// "slice <L> <W>" answers the W + 1 bounds slice(0) .. slice(W) on one line, "form <world>" answers "gathered" or "local".
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>

#include "../csrc/route_host.h"
#include "../csrc/stage_host.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "slice") {
      unsigned long long L = 0, W = 0;
      if (!(in >> L >> W) || W < 1) {
        std::cerr << "topic_sums_slice_main: bad line: " << line << "\n";
        return 2;
      }
      for (unsigned long long q = 0; q <= W; ++q) std::cout << (q ? " " : "") << topic_sums_slice(L, W, q);
      std::cout << "\n";
    } else if (cmd == "form") {
      int world = 0;
      if (!(in >> world)) {
        std::cerr << "topic_sums_slice_main: bad line: " << line << "\n";
        return 2;
      }
      std::cout << (route_topic_sums(world) == TOPIC_SUMS_GATHERED ? "gathered" : "local") << "\n";
    } else {
      std::cerr << "topic_sums_slice_main: unknown command: " << line << "\n";
      return 2;
    }
  }
  return 0;
}
