// isle_amd/host/vocab_host_main.cpp — the rule of isle_hip_prune_vocab (../csrc/vocab_host.h) applied to a script on stdin, one JSON object
// per command on stdout: no library, no GPU (tests/test_vocab_rule_cpu.py builds it with the address and undefined-behaviour sanitizers and
// states every expected value itself).  A count goes in and out as its 32 bits, as an unsigned decimal integer; <k ...> is a count followed
// by that many values.
//   key df w                                                          vocab_key
//   parts V                                                           vocab_df_parts, and VOCAB_DF_PART
//   args has_A min_df max_df keep_n docs_global                       vocab_check_args: the refusal's text, empty = accepted
//   rule min_df max_df keep_n docs_global <V df>                      vocab_rule on a table: text, remap, kept_words
//   prune min_df max_df keep_n docs_global V <D + 1 offsets> <rows> <count bits>
//                                                                     df of the CSC, the checks, the rule and the pruned CSC: what the device call answers
#include <iostream>

#include "../csrc/vocab_host.h"

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
template <class T>
void put_list(const char* name, const std::vector<T>& v, bool last = false) {
  std::cout << "\"" << name << "\": [";
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? ", " : "") << (long long)v[i];
  std::cout << "]" << (last ? "" : ", ");
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "key") {
      const uint32_t df = take<uint32_t>(), w = take<uint32_t>();
      std::cout << "{\"cmd\": \"key\", \"key\": " << (unsigned long long)vocab_key(df, w) << "}\n";
    } else if (cmd == "parts") {
      std::cout << "{\"cmd\": \"parts\", \"parts\": " << vocab_df_parts(take<uint64_t>()) << ", \"part\": " << VOCAB_DF_PART << "}\n";
    } else if (cmd == "args") {
      const int has_A = take<int>();
      const uint64_t min_df = take<uint64_t>(), max_df = take<uint64_t>(), keep_n = take<uint64_t>(), docs = take<uint64_t>();
      std::cout << "{\"cmd\": \"args\", \"text\": \"" << vocab_check_args(has_A != 0, min_df, max_df, keep_n, docs) << "\"}\n";
    } else if (cmd == "rule") {
      const uint64_t min_df = take<uint64_t>(), max_df = take<uint64_t>(), keep_n = take<uint64_t>(), docs = take<uint64_t>();
      const std::vector<uint32_t> df = take_list<uint32_t>();
      std::vector<uint32_t> remap, kept;
      std::string text = vocab_check_args(true, min_df, max_df, keep_n, docs);
      if (text.empty()) text = vocab_rule(df.data(), df.size(), min_df, max_df, keep_n, docs, remap, kept);
      std::cout << "{\"cmd\": \"rule\", \"text\": \"" << text << "\", ";
      put_list("remap", remap);
      put_list("kept_words", kept, true);
      std::cout << "}\n";
    } else if (cmd == "prune") {
      const uint64_t min_df = take<uint64_t>(), max_df = take<uint64_t>(), keep_n = take<uint64_t>(), docs = take<uint64_t>(), V = take<uint64_t>();
      const std::vector<int64_t> offs = take_list<int64_t>();
      const std::vector<uint32_t> rows = take_list<uint32_t>(), bits = take_list<uint32_t>();
      const uint64_t D = offs.size() - 1;
      std::vector<uint32_t> df((size_t)V, 0), remap, kept, new_bits, new_rows;
      std::vector<int64_t> new_offs;
      uint64_t emptied = 0;
      vocab_df_host(D, offs.data(), rows.data(), df.data());
      std::string text = vocab_check_args(true, min_df, max_df, keep_n, docs);
      if (text.empty()) text = vocab_rule(df.data(), V, min_df, max_df, keep_n, docs, remap, kept);
      if (text.empty()) emptied = vocab_prune_csc_host(D, offs.data(), bits.data(), rows.data(), remap.data(), new_offs, new_bits, new_rows);
      else kept.clear();
      std::cout << "{\"cmd\": \"prune\", \"text\": \"" << text << "\", \"docs_emptied\": " << (unsigned long long)emptied << ", ";
      put_list("df", df);
      put_list("kept_words", kept);
      put_list("offs", new_offs);
      put_list("rows", new_rows);
      put_list("counts", new_bits, true);
      std::cout << "}\n";
    } else {
      std::cerr << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
