// isle_amd/host/topdocs_host_main.cpp — the rule of isle_hip_topic_top_docs (../csrc/topdocs_host.h) applied to a script on stdin, one JSON
// object per command on stdout: no library, no GPU (tests/test_topdocs_rule_cpu.py builds it with the address and undefined-behaviour
// sanitizers and states every expected value itself).  A float goes in and out as its 32 bits, as an unsigned decimal integer; <k ...> is a
// count followed by that many values.
//   ord <k bits>                                                    topdocs_ord of every pattern, and topdocs_unord of that
//   key bits doc                                                    topdocs_key, and the way back
//   args source num_topics n world doc_base rows                    topdocs_check_args: the refusal's text, empty = accepted
//   lds num_topics                                                  topdocs_bins_in_lds
//   fault topic num_topics first_of_row topic_before                topdocs_entry_fault
//   select T n doc_base <rows + 1 offsets> <topics> <value bits>    topdocs_select_host, the statement of the rule
//   rounds T n doc_base <offsets> <topics> <value bits> <W + 1 cuts> the device's procedure over W simulated ranks, share q = rows [cut q, cut q + 1)
#include <iostream>

#include "../csrc/topdocs_host.h"

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

void lists(const char* cmd, bool rounds) {
  const uint32_t T = take<uint32_t>(), n = take<uint32_t>();
  const uint64_t doc_base = take<uint64_t>();
  const std::vector<int64_t> off = take_list<int64_t>();
  const std::vector<uint32_t> topic = take_list<uint32_t>(), bits = take_list<uint32_t>();
  const uint64_t rows = off.size() - 1;
  std::vector<uint32_t> docs((size_t)T * n), values((size_t)T * n), counts(T);
  std::vector<uint64_t> entries(T);
  if (rounds) {
    const std::vector<uint64_t> cut = take_list<uint64_t>();
    topdocs_rounds_host(T, n, doc_base, rows, off.data(), topic.data(), bits.data(), cut, docs.data(), values.data(), counts.data(), entries.data());
  } else {
    topdocs_select_host(T, n, doc_base, rows, off.data(), topic.data(), bits.data(), docs.data(), values.data(), counts.data(), entries.data());
  }
  std::cout << "{\"cmd\": \"" << cmd << "\", ";
  put_list("docs", docs);
  put_list("values", values);
  put_list("counts", counts);
  put_list("entries", entries, true);
  std::cout << "}\n";
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "ord") {
      const std::vector<uint32_t> b = take_list<uint32_t>();
      std::vector<uint32_t> o, back;
      for (uint32_t x : b) {
        o.push_back(topdocs_ord(x));
        back.push_back(topdocs_unord(o.back()));
      }
      std::cout << "{\"cmd\": \"ord\", ";
      put_list("ord", o);
      put_list("back", back, true);
      std::cout << "}\n";
    } else if (cmd == "key") {
      const uint32_t bits = take<uint32_t>(), doc = take<uint32_t>();
      const uint64_t k = topdocs_key(bits, doc);
      std::cout << "{\"cmd\": \"key\", \"key\": " << (unsigned long long)k << ", \"doc\": " << topdocs_key_doc(k) << ", \"bits\": " << topdocs_key_bits(k) << "}\n";
    } else if (cmd == "args") {
      const int source = take<int>(), T = take<int>(), n = take<int>(), world = take<int>();
      const uint64_t doc_base = take<uint64_t>(), rows = take<uint64_t>();
      std::cout << "{\"cmd\": \"args\", \"text\": \"" << topdocs_check_args(source, T, n, world, doc_base, rows) << "\"}\n";
    } else if (cmd == "lds") {
      std::cout << "{\"cmd\": \"lds\", \"lds\": " << (topdocs_bins_in_lds(take<uint64_t>()) ? 1 : 0) << "}\n";
    } else if (cmd == "fault") {
      const uint32_t topic = take<uint32_t>(), T = take<uint32_t>(), first = take<uint32_t>(), before = take<uint32_t>();
      std::cout << "{\"cmd\": \"fault\", \"what\": " << topdocs_entry_fault(topic, T, first != 0, before) << "}\n";
    } else if (cmd == "select") {
      lists("select", false);
    } else if (cmd == "rounds") {
      lists("rounds", true);
    } else {
      std::cerr << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
