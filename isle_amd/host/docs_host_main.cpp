// isle_amd/host/docs_host_main.cpp — the rule of isle_hip_prune_docs (../csrc/docs_host.h) applied to a script on stdin, one JSON object per
// command on stdout: no library, no GPU (tests/test_docs_rule_cpu.py builds it with the address and undefined-behaviour sanitizers and
// states every expected value itself).  A count goes in and out as its 32 bits, as an unsigned decimal integer; <k ...> is a count followed
// by that many values.
//   consts                                                            DOCS_DROPPED, DOCS_NARROW_BITS, the ISLE_DOC_HASH_* values
//   hash <rows> <count bits>                                          docs_hash_host of one document, and its narrow cut
//   fails words tokens min_words max_words min_tokens max_tokens      docs_fails
//   args who has_A min_words max_words min_tokens max_tokens drop_duplicates world
//                                                                     docs_check_args: the refusal's text, empty = accepted
//   prune min_words max_words min_tokens max_tokens drop_duplicates doc_offset <D + 1 offsets> <rows> <count bits>
//                                                                     lengths, first-of-its-kind over all documents, the checks, the rule and the
//                                                                     pruned CSC: what the device calls answer
#include <iostream>

#include "../csrc/docs_host.h"

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
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? ", " : "") << (unsigned long long)v[i];
  std::cout << "]" << (last ? "" : ", ");
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "consts") {
      std::cout << "{\"cmd\": \"consts\", \"dropped\": " << DOCS_DROPPED << ", \"narrow_bits\": " << DOCS_NARROW_BITS << ", \"forms\": [" << DOC_HASH_AUTO << ", "
                << DOC_HASH_FULL << ", " << DOC_HASH_NARROW << "], \"key_bits\": [" << docs_key_bits(false) << ", " << docs_key_bits(true) << "]}\n";
    } else if (cmd == "hash") {
      const std::vector<uint32_t> rows = take_list<uint32_t>(), bits = take_list<uint32_t>();
      const uint64_t h = docs_hash_host(rows.data(), bits.data(), 0, (int64_t)rows.size());
      std::cout << "{\"cmd\": \"hash\", \"hash\": " << (unsigned long long)docs_hash_cut(h, false) << ", \"narrow\": " << (unsigned long long)docs_hash_cut(h, true)
                << "}\n";
    } else if (cmd == "fails") {
      const uint64_t w = take<uint64_t>(), t = take<uint64_t>(), a = take<uint64_t>(), b = take<uint64_t>(), c = take<uint64_t>(), d = take<uint64_t>();
      std::cout << "{\"cmd\": \"fails\", \"fails\": " << docs_fails(w, t, a, b, c, d) << "}\n";
    } else if (cmd == "args") {
      const std::string who = take<std::string>();
      const int has_A = take<int>();
      DocsBounds b;
      b.min_words = take<uint64_t>(), b.max_words = take<uint64_t>(), b.min_tokens = take<uint64_t>(), b.max_tokens = take<uint64_t>();
      const int dups = take<int>(), world = take<int>();
      std::cout << "{\"cmd\": \"args\", \"text\": \"" << docs_check_args(who.c_str(), has_A != 0, b, dups, world) << "\"}\n";
    } else if (cmd == "prune") {
      DocsBounds b;
      b.min_words = take<uint64_t>(), b.max_words = take<uint64_t>(), b.min_tokens = take<uint64_t>(), b.max_tokens = take<uint64_t>();
      const int dups = take<int>();
      const uint64_t doc_offset = take<uint64_t>();
      const std::vector<int64_t> offs = take_list<int64_t>();
      const std::vector<uint32_t> rows = take_list<uint32_t>(), bits = take_list<uint32_t>();
      const uint64_t D = offs.size() - 1;
      std::vector<uint32_t> words, all_first, keep, first, kept_docs, new_bits, new_rows;
      std::vector<uint64_t> tokens;
      std::vector<int64_t> new_offs;
      uint64_t dropped[3] = {0, 0, 0};
      docs_lengths_host(D, offs.data(), bits.data(), words, tokens);
      const uint64_t n_dup = docs_first_of_host(D, offs.data(), bits.data(), rows.data(), all_first);
      std::string text = docs_check_args("prune_docs", true, b, dups, 1);
      if (text.empty()) {
        if (!docs_rule(D, offs.data(), bits.data(), rows.data(), b, dups, keep, first, dropped)) text = docs_none_kept(b, dups);
        else docs_prune_csc_host(D, offs.data(), bits.data(), rows.data(), keep.data(), doc_offset, kept_docs, new_offs, new_bits, new_rows);
      }
      std::cout << "{\"cmd\": \"prune\", \"text\": \"" << text << "\", \"n_duplicates\": " << (unsigned long long)n_dup << ", ";
      put_list("words", words);
      put_list("tokens", tokens);
      put_list("all_first_of", all_first);
      put_list("first_of", first);
      put_list("dropped", std::vector<uint64_t>(dropped, dropped + 3));
      put_list("kept_docs", kept_docs);
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
