// isle_amd/host/post_select_main.cpp — the host rules of the distributed radix select of the downstream stage (../csrc/stage_host.h
// select_digit, select_mask, select_chunks / select_chunk; ../csrc/route_host.h route_post_select) applied to a script on stdin, one JSON
// object per command on stdout: no library, no GPU (tests/test_post_select_rule_cpu.py builds it with the address and undefined-behaviour
// sanitizers and states every expected value itself).  A float goes in and out as its 32 bits; <n ...> is a count followed by that many
// values.
//   pick remaining <256 bins>                 select_digit on exactly 256 counters
//   select rank <p parts>, each <n values>    the four passes over a segment whose values lie in p parts: per pass and part the bins of the
//                                             values under the prefix (what post_select_hist_k counts), their sum, select_digit on the sum
//   chunks nslots chunk_slots                 select_chunks, and select_chunk of every chunk
//   plan                                      SELECT_BINS_BYTES, SELECT_CHUNK_SLOTS
//   form world                                route_post_select
#include <iostream>

#include "../csrc/route_host.h"
#include "../csrc/stage_host.h"

namespace {

template <class T>
T take() {
  T v = T();
  std::cin >> v;
  return v;
}
template <class T>
std::vector<T> take_list() {
  std::vector<T> v(take<size_t>());
  for (T& x : v) std::cin >> x;
  return v;
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    std::printf("{\"cmd\": \"%s\", ", cmd.c_str());
    if (cmd == "pick") {
      const uint32_t remaining = take<uint32_t>();
      const std::vector<uint32_t> bins = take_list<uint32_t>();  // exactly what the caller holds: a read past bin 255 is the sanitizer's to find
      if (bins.size() != 256) {
        std::fprintf(stderr, "post_select_main: pick takes 256 bins\n");
        return 2;
      }
      const SelectPick p = select_digit(bins.data(), remaining);
      std::printf("\"digit\": %u, \"remaining\": %u", p.digit, p.remaining);
    } else if (cmd == "select") {
      uint32_t remaining = take<uint32_t>();
      std::vector<std::vector<uint32_t>> parts(take<size_t>());
      for (auto& part : parts) part = take_list<uint32_t>();
      uint32_t prefix = 0;
      for (int shift = 24; shift >= 0; shift -= 8) {
        std::vector<uint32_t> sum(256, 0u);
        for (const auto& part : parts) {
          std::vector<uint32_t> bins(256, 0u);  // one rank's
          for (uint32_t key : part)
            if ((key & select_mask(shift)) == prefix) bins[(key >> shift) & 255u]++;
          for (int d = 0; d < 256; ++d) sum[d] += bins[d];
        }
        const SelectPick p = select_digit(sum.data(), remaining);
        prefix |= p.digit << shift;
        remaining = p.remaining;
      }
      std::printf("\"value\": %u, \"remaining\": %u", prefix, remaining);
    } else if (cmd == "chunks") {
      const uint64_t nslots = take<uint64_t>(), chunk = take<uint64_t>();
      const uint64_t n = select_chunks(nslots, chunk);
      std::printf("\"n\": %llu, \"chunks\": [", (unsigned long long)n);
      for (uint64_t i = 0; i < n; ++i) {
        const SlotChunk s = select_chunk(nslots, chunk, i);
        std::printf(i ? ",[%llu,%llu]" : "[%llu,%llu]", (unsigned long long)s.first, (unsigned long long)s.count);
      }
      std::printf("]");
    } else if (cmd == "plan") {
      std::printf("\"bins_bytes\": %llu, \"chunk_slots\": %llu", (unsigned long long)SELECT_BINS_BYTES, (unsigned long long)SELECT_CHUNK_SLOTS);
    } else if (cmd == "form") {
      std::printf("\"histogram\": %d", route_post_select(take<int>()) == POST_SELECT_HISTOGRAM ? 1 : 0);
    } else {
      std::fprintf(stderr, "post_select_main: unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::printf("}\n");
    if (!std::cin) {
      std::fprintf(stderr, "post_select_main: %s: input ended or did not parse\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
