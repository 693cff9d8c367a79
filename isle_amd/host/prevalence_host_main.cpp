// isle_amd/host/prevalence_host_main.cpp — the rule of isle_hip_topic_prevalence (../csrc/prevalence_host.h) applied to a script on stdin, one
// JSON object per command on stdout: no library, no GPU (tests/test_prevalence_rule_cpu.py builds it and states every expected value
// itself).  A float goes in as its 32 bits, a double comes out as its 64 bits, as unsigned decimal integers; <k ...> is a count followed by
// that many values; <groups> is empty (no labels) or one label per row.
//   ok <k bits>                                                              prev_weight_ok of every pattern
//   tile num_topics asked                                                    prev_tile
//   levels n                                                                 prev_levels
//   lds num_groups num_topics                                                prev_hist_in_lds
//   args source num_topics num_groups normalise has_groups world rows        prevalence_check_args: the refusal's text, empty = accepted
//   form f                                                                   prevalence_check_form
//   faults num_topics num_groups <rows + 1 offsets> <topics> <weight bits> <groups>
//                                                                            prevalence_first_faults and the text the call refuses with
//   prev num_topics num_groups normalise <rows + 1 offsets> <topics> <weight bits> <groups>
//                                                                            prevalence_host, the statement of the rule
#include <cstring>
#include <iostream>

#include "../csrc/prevalence_host.h"

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
std::vector<float> take_floats() {
  const std::vector<uint32_t> b = take_list<uint32_t>();
  std::vector<float> f(b.size());
  if (!b.empty()) std::memcpy(f.data(), b.data(), b.size() * sizeof(float));
  return f;
}
template <class T>
void put_list(const char* name, const std::vector<T>& v, bool last = false) {
  std::cout << "\"" << name << "\": [";
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? ", " : "") << (unsigned long long)v[i];
  std::cout << "]" << (last ? "" : ", ");
}
void put_text(const char* cmd, const std::string& text) { std::cout << "{\"cmd\": \"" << cmd << "\", \"text\": \"" << text << "\"}\n"; }

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "ok") {
      const std::vector<float> w = take_floats();
      std::vector<uint32_t> ok;
      for (float x : w) ok.push_back(prev_weight_ok(x) ? 1 : 0);
      std::cout << "{\"cmd\": \"ok\", ";
      put_list("ok", ok, true);
      std::cout << "}\n";
    } else if (cmd == "tile") {
      const uint32_t k = take<uint32_t>();
      const int asked = take<int>();
      std::cout << "{\"cmd\": \"tile\", \"tile\": " << prev_tile(k, asked) << "}\n";
    } else if (cmd == "levels") {
      std::cout << "{\"cmd\": \"levels\", \"levels\": " << prev_levels(take<uint64_t>()) << "}\n";
    } else if (cmd == "lds") {
      const uint64_t G = take<uint64_t>(), k = take<uint64_t>();
      std::cout << "{\"cmd\": \"lds\", \"lds\": " << (prev_hist_in_lds(G, k) ? 1 : 0) << "}\n";
    } else if (cmd == "args") {
      const int source = take<int>(), k = take<int>();
      const uint64_t G = take<uint64_t>();
      const int normalise = take<int>(), has_groups = take<int>(), world = take<int>();
      const uint64_t rows = take<uint64_t>();
      put_text("args", prevalence_check_args(source, k, G, normalise, has_groups != 0, world, rows));
    } else if (cmd == "form") {
      put_text("form", prevalence_check_form(take<int>()));
    } else if (cmd == "faults" || cmd == "prev") {
      const bool prev = cmd == "prev";
      const uint32_t k = take<uint32_t>(), G = take<uint32_t>();
      const int normalise = prev ? take<int>() : 0;
      const std::vector<int64_t> off = take_list<int64_t>();
      const std::vector<uint32_t> topic = take_list<uint32_t>();
      const std::vector<float> w = take_floats();
      const std::vector<uint32_t> groups = take_list<uint32_t>();
      const uint64_t rows = off.size() - 1;
      const uint32_t* const gp = groups.empty() ? nullptr : groups.data();
      if (!prev) {
        uint64_t bad_row = 0, bad_entry = 0;
        prevalence_first_faults(k, rows, off.data(), topic.data(), w.data(), gp, G, &bad_row, &bad_entry);
        std::string text;
        if (bad_row != ~0ull) text = prevalence_label_text(bad_row, gp[bad_row], G);
        else if (bad_entry != ~0ull) {
          const uint64_t e = bad_entry >> 2;
          const uint64_t row = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)e) - off.begin()) - 1;
          text = prevalence_entry_text((unsigned)(bad_entry & 3), e, row, topic[e], w[e], k);
        }
        put_text("faults", text);
        continue;
      }
      const size_t cells = (size_t)G * k;
      std::vector<uint64_t> docs(G), count(cells), dominant(cells), bits(cells);
      std::vector<double> sum(cells);
      uint64_t none = 0;
      prevalence_host(k, rows, off.data(), topic.data(), w.data(), gp, G, normalise, docs.data(), &none, count.data(), dominant.data(), sum.data());
      if (cells) std::memcpy(bits.data(), sum.data(), cells * sizeof(double));
      std::cout << "{\"cmd\": \"prev\", \"unlabelled\": " << (unsigned long long)none << ", ";
      put_list("docs", docs);
      put_list("count", count);
      put_list("dominant", dominant);
      put_list("sum", bits, true);
      std::cout << "}\n";
    } else {
      std::cerr << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
