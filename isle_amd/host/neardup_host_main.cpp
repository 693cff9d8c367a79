// isle_amd/host/neardup_host_main.cpp — the rule of isle_hip_prune_near_docs (../csrc/neardup_host.h) applied to a script on stdin, one JSON
// object per command on stdout: no library, no GPU (tests/test_neardup_rule_cpu.py builds it with the address and undefined-behaviour
// sanitizers and states every expected value itself).  A count goes in and out as its 32 bits; <k ...> is a count followed by that many
// values.  64-bit values go out as decimal integers.
//   consts                                                   the ND_KEY_* values, the limits, the empty signature
//   hash i w                                                 nd_hash(i, w)
//   similar inter na nb num den                              nd_lengths_allow(na, nb) and nd_similar
//   args who has_A num den bands rows_per_band world         nd_check_args: the refusal's text, empty = accepted
//   pairs D <a> <b>                                          nd_first_bad_pair, and nd_bad_pair's text where there is one
//   rule narrow with_sig num den bands rows_per_band doc_offset <D + 1 offsets> <rows> <count bits> <a> <b>
//                                                            signatures, band keys, the pairs' sizes, the resolution, the roots and the
//                                                            pruned CSC: what the device calls answer (with_sig == 0: the signatures
//                                                            and keys are used, not printed)
#include <iostream>

#include "../csrc/neardup_host.h"

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
      std::cout << "{\"cmd\": \"consts\", \"forms\": [" << ND_KEY_AUTO << ", " << ND_KEY_FULL << ", " << ND_KEY_NARROW << "], \"limits\": [" << ND_MAX_BANDS << ", "
                << ND_MAX_ROWS << ", " << ND_MAX_H << ", " << ND_MAX_DEN << "], \"empty_sig\": " << (unsigned long long)ND_EMPTY_SIG << ", \"narrow_bits\": "
                << DOCS_NARROW_BITS << "}\n";
    } else if (cmd == "hash") {
      const uint32_t i = take<uint32_t>(), w = take<uint32_t>();
      std::cout << "{\"cmd\": \"hash\", \"hash\": " << (unsigned long long)nd_hash(i, w) << "}\n";
    } else if (cmd == "similar") {
      const uint64_t inter = take<uint64_t>(), na = take<uint64_t>(), nb = take<uint64_t>(), num = take<uint64_t>(), den = take<uint64_t>();
      std::cout << "{\"cmd\": \"similar\", \"allow\": " << (int)nd_lengths_allow(na, nb, num, den) << ", \"similar\": " << (int)nd_similar(inter, na, nb, num, den) << "}\n";
    } else if (cmd == "args") {
      const std::string who = take<std::string>();
      const int has_A = take<int>();
      const uint64_t num = take<uint64_t>(), den = take<uint64_t>();
      const long long bands = take<long long>(), rpb = take<long long>();
      const int world = take<int>();
      std::cout << "{\"cmd\": \"args\", \"text\": \"" << nd_check_args(who.c_str(), has_A != 0, num, den, bands, rpb, world) << "\"}\n";
    } else if (cmd == "pairs") {
      const uint64_t D = take<uint64_t>();
      const std::vector<uint32_t> a = take_list<uint32_t>(), b = take_list<uint32_t>();
      const uint64_t bad = nd_first_bad_pair(a.size(), a.data(), b.data(), D);
      std::cout << "{\"cmd\": \"pairs\", \"bad\": " << (unsigned long long)bad << ", \"text\": \"" << (bad < a.size() ? nd_bad_pair(bad, a[bad], b[bad], D) : std::string())
                << "\"}\n";
    } else if (cmd == "rule") {
      const int narrow = take<int>(), with_sig = take<int>();
      const uint64_t num = take<uint64_t>(), den = take<uint64_t>();
      const int bands = take<int>(), rpb = take<int>();
      const uint64_t doc_offset = take<uint64_t>();
      const std::vector<int64_t> offs = take_list<int64_t>();
      const std::vector<uint32_t> rows = take_list<uint32_t>(), bits = take_list<uint32_t>(), a = take_list<uint32_t>(), b = take_list<uint32_t>();
      const uint64_t D = offs.size() - 1;
      const std::string text = nd_check_args("doc_near_duplicates", true, num, den, bands, rpb, 1);
      std::vector<uint64_t> sig, keys;
      std::vector<uint32_t> inter(a.size()), uni(a.size()), kept_docs, new_bits, new_rows;
      std::vector<int64_t> new_offs;
      NdResult r;
      if (text.empty()) {
        nd_signatures_host(D, offs.data(), rows.data(), bands * rpb, sig);
        nd_keys_host(D, sig.data(), bands, rpb, keys);
        for (size_t i = 0; i < a.size(); ++i) nd_jaccard_host(offs.data(), rows.data(), a[i], b[i], &inter[i], &uni[i]);
        nd_rule(D, offs.data(), rows.data(), keys.data(), bands, narrow != 0, num, den, r);
        docs_prune_csc_host(D, offs.data(), bits.data(), rows.data(), r.keep.data(), doc_offset, kept_docs, new_offs, new_bits, new_rows);
      }
      std::cout << "{\"cmd\": \"rule\", \"text\": \"" << text << "\", \"n_dropped\": " << (unsigned long long)r.n_dropped << ", \"pairs_tested\": "
                << (unsigned long long)r.pairs_tested << ", \"rounds\": " << (unsigned long long)r.rounds << ", ";
      put_list("sig", with_sig ? sig : std::vector<uint64_t>());
      put_list("keys", with_sig ? keys : std::vector<uint64_t>());
      put_list("inter", inter);
      put_list("uni", uni);
      put_list("parent", r.parent);
      put_list("first_of", r.first_of);
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
