// isle_amd/host/stage_host_main.cpp — the host rules of the stages either side of the hot path (../csrc/stage_host.h) applied to a script on
// stdin, one JSON object per command on stdout: no library, no GPU (tests/test_stage_host_cpu.py builds it with the address and
// undefined-behaviour sanitizers and states every expected value itself).  A float goes in and out as its 32 bits, a double as its 64 bits,
// both as unsigned decimal integers; <k ...> is a count followed by that many values.
//   avg tokens nz_docs                        corpus_avg, then hist_maxv of it
//   maxv <avg>                                hist_maxv of a given average
//   counts nz_docs num_topics                 threshold_counts
//   keys seed doc_offset <n weights>          sample_keys: documents doc_offset .. doc_offset + n - 1
//   pad dmax <n keys>                         sample_pad
//   pivot <rate> <n keys>                     sample_pivot (keys with or without padding)
//   mask <pivot> <n keys>                     drop_mask
//   place rank <world kept>                   shard_placement
//   coh T M vocab <T*M words> <eps> <k cnt>   CoherencePlan, and with k = |U| + |P| counts coherence_sums
//   top5 m <n runs>                           top_five_count
//   div kp <k dist>                           diversity_average
//   line pos <hex of the text | ->            line_of_byte
#include <cstring>
#include <iostream>

#include "../csrc/stage_host.h"

namespace {

uint32_t f2b(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}
float b2f(uint32_t b) {
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}
unsigned long long d2b(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  return b;
}
double b2d(unsigned long long b) {
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}
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
std::vector<float> take_floats() {
  std::vector<float> v;
  for (uint32_t b : take_list<uint32_t>()) v.push_back(b2f(b));
  return v;
}
template <class V, class F>
void put(const char* name, const V& v, F as) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%llu" : "%llu", (unsigned long long)as(v[i]));
  std::printf("]");
}
unsigned long long same(unsigned long long v) { return v; }

void coherence() {
  const size_t T = take<size_t>(), M = take<size_t>();
  const unsigned long long vocab = take<unsigned long long>();
  std::vector<uint32_t> words(T * M);
  for (uint32_t& w : words) std::cin >> w;
  const double eps = b2d(take<unsigned long long>());
  const std::vector<uint32_t> cnt = take_list<uint32_t>();
  const CoherencePlan pl(words.data(), T, M, vocab);
  if (!pl.refused.empty()) {
    std::printf("\"refused\": \"%s\"", pl.refused.c_str());
    return;
  }
  put("U", pl.U, same), std::printf(", ");
  put("loc", pl.loc, same), std::printf(", ");
  put("keys", pl.keys, same), std::printf(", ");
  put("P", pl.P, same), std::printf(", ");
  put("part_off", pl.part_off, same), std::printf(", ");
  put("part_hi", pl.part_hi, same);
  if (cnt.size() != pl.U.size() + pl.P.size()) return;
  // exactly the sizes the entry's caller passes: an overrun is the sanitizer's to find
  std::vector<double> coh(T);
  std::vector<uint64_t> df(T * M), cdf(T * pl.npt);
  coherence_sums(pl, cnt.data(), eps, coh.data(), df.data(), cdf.data());
  std::vector<double> coh_only(T);
  coherence_sums(pl, cnt.data(), eps, coh_only.data(), nullptr, nullptr);
  std::printf(", \"same_without_outputs\": %s, ", std::memcmp(coh.data(), coh_only.data(), T * sizeof(double)) == 0 ? "true" : "false");
  put("coherence", coh, d2b), std::printf(", ");
  put("doc_freq", df, same), std::printf(", ");
  put("co_doc_freq", cdf, same);
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    std::printf("{\"cmd\": \"%s\", ", cmd.c_str());
    if (cmd == "avg" || cmd == "maxv") {
      float avg;
      if (cmd == "avg") {
        const uint64_t tokens = take<uint64_t>(), nz = take<uint64_t>();
        avg = corpus_avg(tokens, nz);
      } else {
        avg = b2f(take<uint32_t>());
      }
      uint32_t maxv = 0;
      const bool ok = hist_maxv(avg, &maxv);
      std::printf("\"avg\": %u, \"ok\": %s, \"maxv\": %u", f2b(avg), ok ? "true" : "false", maxv);
    } else if (cmd == "counts") {
      const uint64_t nz = take<uint64_t>(), k = take<uint64_t>();
      const ThresholdCounts n = threshold_counts(nz, k);
      std::printf("\"gr\": %llu, \"eq\": %llu", (unsigned long long)n.gr, (unsigned long long)n.eq);
    } else if (cmd == "keys") {
      const uint64_t seed = take<uint64_t>(), doc_offset = take<uint64_t>();
      put("keys", sample_keys(seed, doc_offset, take_floats()), f2b);
    } else if (cmd == "pad") {
      const uint64_t dmax = take<uint64_t>();
      put("keys", sample_pad(take_floats(), dmax), f2b);
    } else if (cmd == "pivot") {
      const double rate = b2d(take<unsigned long long>());
      std::vector<float> dice = take_floats();
      std::printf("\"pivot\": %u", f2b(sample_pivot(rate, dice)));
    } else if (cmd == "mask") {
      const float pivot = b2f(take<uint32_t>());
      const std::vector<float> key = take_floats();
      const std::vector<uint8_t> drop = drop_mask(key, pivot);
      std::printf("\"n\": %zu, \"slots\": %zu, ", key.size(), drop.size());
      put("drop", drop, same);
    } else if (cmd == "place") {
      const int rank = take<int>();
      const ShardPlace s = shard_placement(rank, take_list<uint64_t>());
      std::printf("\"b_off\": %llu, \"b_glob\": %llu", (unsigned long long)s.b_off, (unsigned long long)s.b_glob);
    } else if (cmd == "coh") {
      coherence();
    } else if (cmd == "top5") {
      const int32_t m = take<int32_t>();
      const std::vector<uint64_t> runs = take_list<uint64_t>();  // an empty list has no storage: the rule must not read it
      std::printf("\"num\": %llu", (unsigned long long)top_five_count(runs.empty() ? nullptr : runs.data(), runs.size(), m));
    } else if (cmd == "div") {
      const uint32_t kp = take<uint32_t>();
      std::vector<double> dist;
      for (unsigned long long b : take_list<unsigned long long>()) dist.push_back(b2d(b));
      std::printf("\"avg\": %llu", d2b(diversity_average(dist.data(), (uint32_t)dist.size(), kp)));
    } else if (cmd == "line") {
      const uint64_t pos = take<uint64_t>();
      const std::string hex = take<std::string>();
      std::vector<char> text;  // exactly nbytes, no terminator: a read past the end is the sanitizer's to find
      for (size_t i = 0; hex != "-" && i + 1 < hex.size(); i += 2) text.push_back((char)std::stoi(hex.substr(i, 2), nullptr, 16));
      std::printf("\"line\": %llu", (unsigned long long)line_of_byte(text.empty() ? nullptr : text.data(), text.size(), pos));
    } else {
      std::fprintf(stderr, "stage_host_main: unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::printf("}\n");
    if (!std::cin) {
      std::fprintf(stderr, "stage_host_main: %s: input ended or did not parse\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
