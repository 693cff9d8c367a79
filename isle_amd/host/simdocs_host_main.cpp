// isle_amd/host/simdocs_host_main.cpp — the rule of isle_hip_similar_docs (../csrc/simdocs_host.h) and the home of its query table
// (../csrc/route_host.h, route_simdocs_table) applied to a script on stdin, one JSON object per command on stdout: no library, no GPU
// (tests/test_simdocs_rule_cpu.py builds it and states every expected value itself).  A float goes in and out as its 32 bits, as an unsigned
// decimal integer; <k ...> is a count followed by that many values.
//   ok <k bits>                                                      simdocs_weight_ok of every pattern
//   qp Q                                                             simdocs_qp
//   args source measure num_topics n Q world doc_base rows           simdocs_check_args: the refusal's text, empty = accepted
//   form f                                                           simdocs_check_form
//   qrows rows <k query_rows>                                        simdocs_check_query_rows
//   queries num_topics <Q + 1 offsets> <topics> <weight bits>        simdocs_check_queries
//   table Q num_topics asked                                         route_simdocs_table: 0 LDS, 1 global
//   select measure n doc_base <rows + 1 offsets> <topics> <weight bits> <Q + 1 offsets> <topics> <weight bits> <0 or Q excluded documents>
//                                                                    simdocs_select_host, the statement of the rule
#include <cstring>
#include <iostream>

#include "../csrc/route_host.h"
#include "../csrc/simdocs_host.h"

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
      for (float x : w) ok.push_back(simdocs_weight_ok(x) ? 1 : 0);
      std::cout << "{\"cmd\": \"ok\", ";
      put_list("ok", ok, true);
      std::cout << "}\n";
    } else if (cmd == "qp") {
      std::cout << "{\"cmd\": \"qp\", \"qp\": " << simdocs_qp(take<uint32_t>()) << "}\n";
    } else if (cmd == "args") {
      const int source = take<int>(), measure = take<int>(), T = take<int>(), n = take<int>(), Q = take<int>(), world = take<int>();
      const uint64_t doc_base = take<uint64_t>(), rows = take<uint64_t>();
      put_text("args", simdocs_check_args(source, measure, T, n, Q, world, doc_base, rows));
    } else if (cmd == "form") {
      put_text("form", simdocs_check_form(take<int>()));
    } else if (cmd == "qrows") {
      const uint64_t rows = take<uint64_t>();
      const std::vector<uint64_t> qr = take_list<uint64_t>();
      put_text("qrows", simdocs_check_query_rows(qr.data(), (int)qr.size(), rows));
    } else if (cmd == "queries") {
      const uint32_t T = take<uint32_t>();
      const std::vector<int64_t> off = take_list<int64_t>();
      const std::vector<uint32_t> topic = take_list<uint32_t>();
      const std::vector<float> w = take_floats();
      put_text("queries", simdocs_check_queries((int)off.size() - 1, T, off.data(), topic.data(), w.data()));
    } else if (cmd == "table") {
      const int Q = take<int>();
      const uint64_t T = take<uint64_t>();
      const int asked = take<int>();
      std::cout << "{\"cmd\": \"table\", \"home\": " << (int)route_simdocs_table(Q, T, asked) << "}\n";
    } else if (cmd == "select") {
      const int measure = take<int>();
      const uint32_t n = take<uint32_t>();
      const uint64_t doc_base = take<uint64_t>();
      const std::vector<int64_t> off = take_list<int64_t>();
      const std::vector<uint32_t> topic = take_list<uint32_t>();
      const std::vector<float> w = take_floats();
      const std::vector<int64_t> q_off = take_list<int64_t>();
      const std::vector<uint32_t> q_topic = take_list<uint32_t>();
      const std::vector<float> q_w = take_floats();
      const std::vector<uint32_t> exclude = take_list<uint32_t>();
      const uint32_t Q = (uint32_t)q_off.size() - 1;
      std::vector<uint32_t> docs((size_t)Q * n), scores((size_t)Q * n), counts(Q);
      std::vector<uint64_t> cand(Q);
      simdocs_select_host(measure, n, doc_base, off.size() - 1, off.data(), topic.data(), w.data(), Q, q_off.data(), q_topic.data(), q_w.data(),
                          exclude.empty() ? nullptr : exclude.data(), docs.data(), scores.data(), counts.data(), cand.data());
      std::cout << "{\"cmd\": \"select\", ";
      put_list("docs", docs);
      put_list("scores", scores);
      put_list("counts", counts);
      put_list("candidates", cand, true);
      std::cout << "}\n";
    } else {
      std::cerr << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
