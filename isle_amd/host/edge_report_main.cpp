// isle_amd/host/edge_report_main.cpp — the host statements of the edge-topic stage on a drawn input, without a device and without the
// library: fpsparse_detail::select_edge_pairs_host and trainer_detail::edge_composition_text / edge_top_words_text.  Stand-alone (it
// links nothing), so that tests/test_edge_rule_cpu.py can also build it with -fsanitize=address,undefined.
//   edge_report_main <input> <composition_out> <top_words_out>
// input (raw): int64 n_docs, max_edge_topics, min_docs, num_topics, n_edge, n_edge_words, n_topic_words; int32 top1[n_docs], top2[n_docs];
// uint32 edge_ids[n_edge x n_edge_words]; float edge_w[same]; uint32 topic_ids[num_topics x n_topic_words]; float topic_w[same].  The
// vocabulary is "w<id>".  Exit 3 when the selection does not have n_edge entries (the files are not written then).
#include "trainer_hip.h"

using namespace ISLE;

template <class T>
static bool read_vec(std::ifstream& in, std::vector<T>& v, size_t n) {
  v.resize(n);
  in.read((char*)v.data(), (std::streamsize)(n * sizeof(T)));
  return (bool)in;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::cerr << "usage: edge_report_main <input> <composition_out> <top_words_out>\n";
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  std::vector<int64_t> h;
  if (!read_vec(in, h, 7) || h[0] < 0 || h[3] < 1 || h[4] < 0 || h[5] < 0 || h[6] < 0) {
    std::cerr << "bad header\n";
    return 2;
  }
  const size_t n_docs = (size_t)h[0], k = (size_t)h[3], n_edge = (size_t)h[4], new_ = (size_t)h[5], ntw = (size_t)h[6];
  std::vector<int32_t> t1, t2;
  std::vector<uint32_t> e_ids, t_ids;
  std::vector<float> e_w, t_w;
  if (!read_vec(in, t1, n_docs) || !read_vec(in, t2, n_docs) || !read_vec(in, e_ids, n_edge * new_) || !read_vec(in, e_w, n_edge * new_) ||
      !read_vec(in, t_ids, k * ntw) || !read_vec(in, t_w, k * ntw)) {
    std::cerr << "short input\n";
    return 2;
  }
  std::vector<std::tuple<int, int, uint64_t>> sel;
  uint64_t cand = 0, thr = 0;
  fpsparse_detail::select_edge_pairs_host(t1.data(), t2.data(), n_docs, h[1], (uint64_t)h[2], sel, &cand, &thr);
  std::cout << "candidates " << cand << " threshold " << thr << " selected " << sel.size() << std::endl;
  if (sel.size() != n_edge) return 3;
  uint32_t max_id = 0;
  for (uint32_t id : e_ids) max_id = std::max(max_id, id);
  for (uint32_t id : t_ids) max_id = std::max(max_id, id);
  for (const auto& p : sel)
    if (std::get<0>(p) >= (int)k || std::get<1>(p) >= (int)k) return 2;
  std::vector<std::string> vocab((size_t)max_id + 1);
  for (size_t w = 0; w < vocab.size(); ++w) vocab[w] = "w" + std::to_string(w);
  std::ofstream(argv[2], std::ios::binary) << trainer_detail::edge_composition_text(sel);
  std::ofstream(argv[3], std::ios::binary) << trainer_detail::edge_top_words_text(sel, vocab, e_ids.data(), e_w.data(), new_, t_ids.data(), t_w.data(), ntw);
  return 0;
}
