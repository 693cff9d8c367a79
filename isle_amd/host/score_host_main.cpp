// isle_amd/host/score_host_main.cpp — the rule of isle_hip_score_docs (../csrc/score_host.h) applied to a script on stdin, one JSON object per
// command on stdout: no library, no GPU (tests/test_score_rule_cpu.py builds it and states every expected value itself).  A float goes in
// as its 32 bits and a double as its 64 bits, a double comes out as its 64 bits, as unsigned decimal integers; <k ...> is a count followed
// by that many values.
//   args weights_source entries_source measure normalise <floor bits> ncols   score_check_args: the refusal's text, empty = accepted
//   offsets name <offsets>                                                    score_check_offsets
//   held seed num den doc_offset <docs> <words>                               score_held_out of every (doc_offset + doc, word)
//   total <double bits>                                                       score_total
//   faults ncols vocab <rows + 1 w_offsets> <topics> <weight bits> <rows + 1 offsets> <words> <count bits>
//                                                                             score_first_faults and the text the call refuses with
//   score ncols vocab measure normalise <floor bits> <model bits, vocab x ncols column-major> <w_offsets> <topics> <weight bits>
//         <offsets> <words> <count bits>                                      score_docs_host, the statement of the rule
#include <cstring>
#include <iostream>

#include "../csrc/score_host.h"

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
double take_double() {
  const uint64_t b = take<uint64_t>();
  double d;
  std::memcpy(&d, &b, sizeof(d));
  return d;
}
template <class T>
void put_list(const char* name, const std::vector<T>& v, bool last = false) {
  std::cout << "\"" << name << "\": [";
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? ", " : "") << (unsigned long long)v[i];
  std::cout << "]" << (last ? "" : ", ");
}
void put_bits(const char* name, const std::vector<double>& v, bool last = false) {
  std::vector<uint64_t> b(v.size());
  if (!v.empty()) std::memcpy(b.data(), v.data(), v.size() * sizeof(double));
  put_list(name, b, last);
}
void put_text(const char* cmd, const std::string& text) { std::cout << "{\"cmd\": \"" << cmd << "\", \"text\": \"" << text << "\"}\n"; }

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "args") {
      const int ws = take<int>(), es = take<int>(), measure = take<int>(), normalise = take<int>();
      const double floor = take_double();
      const int ncols = take<int>();
      put_text("args", score_check_args(ws, es, measure, normalise, floor, ncols));
    } else if (cmd == "offsets") {
      const std::string name = take<std::string>();
      const std::vector<int64_t> off = take_list<int64_t>();
      put_text("offsets", score_check_offsets(name.c_str(), off.data(), off.size() - 1));
    } else if (cmd == "held") {
      const uint64_t seed = take<uint64_t>(), num = take<uint64_t>(), den = take<uint64_t>(), base = take<uint64_t>();
      const std::vector<uint64_t> docs = take_list<uint64_t>();
      const std::vector<uint32_t> words = take_list<uint32_t>();
      std::vector<uint32_t> held(docs.size());
      for (size_t i = 0; i < docs.size(); ++i) held[i] = score_held_out(seed, base + docs[i], words[i], num, den) ? 1 : 0;
      std::cout << "{\"cmd\": \"held\", ";
      put_list("held", held, true);
      std::cout << "}\n";
    } else if (cmd == "total") {
      std::vector<double> v(take<size_t>());
      for (double& x : v) x = take_double();
      std::cout << "{\"cmd\": \"total\", ";
      put_bits("total", std::vector<double>(1, score_total(v.data(), v.size())), true);
      std::cout << "}\n";
    } else if (cmd == "faults" || cmd == "score") {
      const bool run = cmd == "score";
      const uint32_t ncols = take<uint32_t>();
      const uint64_t vocab = take<uint64_t>();
      const int measure = run ? take<int>() : 0, normalise = run ? take<int>() : 0;
      const double floor = run ? take_double() : 0.0;
      const std::vector<float> model = run ? take_floats() : std::vector<float>();
      const std::vector<int64_t> w_off = take_list<int64_t>();
      const std::vector<uint32_t> topic = take_list<uint32_t>();
      const std::vector<float> w = take_floats();
      const std::vector<int64_t> off = take_list<int64_t>();
      const std::vector<uint32_t> word = take_list<uint32_t>();
      const std::vector<float> cnt = take_floats();
      const uint64_t rows = off.size() - 1;
      if (!run) {
        uint64_t bad_w = 0, bad_e = 0;
        score_first_faults(ncols, vocab, rows, w_off.data(), topic.data(), w.data(), cnt.data(), word.data(), off.data(), &bad_w, &bad_e);
        std::string text;
        if (bad_w != ~0ull) {
          const uint64_t e = bad_w >> 2;
          const uint64_t row = (uint64_t)(std::upper_bound(w_off.begin(), w_off.end(), (int64_t)e) - w_off.begin()) - 1;
          text = score_weight_text((unsigned)(bad_w & 3), e, row, topic[e], w[e], ncols);
        } else if (bad_e != ~0ull) {
          const uint64_t e = bad_e >> 1;
          const uint64_t row = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)e) - off.begin()) - 1;
          text = score_entry_text((unsigned)(bad_e & 1), e, row, word[e], cnt[e], vocab);
        }
        put_text("faults", text);
        continue;
      }
      std::vector<double> score(rows), tokens(rows), ut(rows), z(word.size());
      std::vector<uint32_t> ue(rows), fl(rows);
      score_docs_host(ncols, vocab, model.data(), rows, w_off.data(), topic.data(), w.data(), cnt.data(), word.data(), off.data(), measure, normalise, floor,
                      score.data(), tokens.data(), ue.data(), ut.data(), fl.data(), z.data());
      std::cout << "{\"cmd\": \"score\", ";
      put_bits("z", z);
      put_bits("score", score);
      put_bits("tokens", tokens);
      put_list("unscored_entries", ue);
      put_bits("unscored_tokens", ut);
      put_list("floored", fl, true);
      std::cout << "}\n";
    } else {
      std::cerr << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
