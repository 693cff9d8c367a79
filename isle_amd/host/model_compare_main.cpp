// isle_amd/host/model_compare_main.cpp — isle_hip_compare_models / isle_hip_match_topics through FPSparseMatrixHip held to ../csrc/match_host.h,
// and ISLETrainer::output_model_comparison as a driver calls it (tests/test_gpu_model_compare_host_cpp.py).
//   model_compare_main check <case_file>
//       the file holds cases in the words of match_host_main's script: "dist V ka kb <a bits> <b bits>" (floats as their 32 bits, every
//       entry an integer multiple of 2^-12 so that every sum is exact) and "match na nb <dist bits>" (doubles as their 64 bits).  A dist
//       case is compared on the device as two host models: the distances must equal model_dist_plain bit for bit (NaN as positions) and
//       the matching must equal match_greedy on them; a match case goes through match_topics and must equal match_greedy.  Status 3
//       otherwise.
//   model_compare_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics>
//       FILE_DATA_LOAD, train, output_cluster_summary, write_model_to_file, then output_model_comparison on the M_hat_catch_sparse just
//       written: TopicMatch.tsv must equal trainer_detail::topic_match_text of a second comparison of the same two resident models byte
//       for byte, and its matching must be match_greedy's on the plain loop's distances of the fetched models.  Status 3 otherwise.  The
//       log directory's name is printed.
//   model_compare_main --time <vocab_size> <cols_a> <cols_b>
//       the median, least and greatest wall time of five comparisons of two generated host models (uploads included), after one warm-up.
#include <chrono>

#include "trainer_hip.h"

#include "../csrc/match_host.h"

using namespace ISLE;

namespace {

uint64_t bits_of(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof(u));
  return u;
}
bool same_doubles(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (std::isnan(a[i]) != std::isnan(b[i]) || (!std::isnan(a[i]) && bits_of(a[i]) != bits_of(b[i]))) return false;
  return true;
}
bool same_match(const FPSparseMatrixHip::TopicMatch& got, const McMatch& want) {
  return got.match_a == want.match_a && got.match_b == want.match_b && same_doubles(got.match_dist, want.match_dist) && got.n_matched == want.n_matched &&
         same_doubles(std::vector<double>(1, got.mean_dist), std::vector<double>(1, want.mean_dist));
}

int check(const char* path) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error(std::string("cannot read ") + path);
  FPSparseMatrixHip m(1, 1);
  std::string cmd;
  int ndist = 0, nmatch = 0;
  while (in >> cmd) {
    if (cmd == "dist") {
      uint64_t V = 0, na = 0, nb = 0;
      int ka = 0, kb = 0;
      in >> V >> ka >> kb >> na;
      std::vector<uint32_t> ab((size_t)na);
      for (uint32_t& x : ab) in >> x;
      in >> nb;
      std::vector<uint32_t> bb((size_t)nb);
      for (uint32_t& x : bb) in >> x;
      if (!in || na != V * (uint64_t)ka || nb != V * (uint64_t)kb) throw std::runtime_error("malformed dist case");
      std::vector<float> a(ab.size()), b(bb.size());
      std::memcpy(a.data(), ab.data(), ab.size() * sizeof(float));
      std::memcpy(b.data(), bb.data(), bb.size() * sizeof(float));
      std::vector<double> want, got;
      model_dist_plain(a.data(), ka, b.data(), kb, V, want);
      const FPSparseMatrixHip::TopicMatch gm = m.compare_models(ISLE_MODEL_HOST, ISLE_MODEL_HOST, &got, a.data(), ka, b.data(), kb, (word_id_t)V);
      if (!same_doubles(got, want) || !same_match(gm, match_greedy(want.data(), ka, kb))) {
        std::cerr << "model_compare_main: dist case " << ndist << " (" << V << " words, " << ka << " x " << kb << ") is not match_host.h's\n";
        return 3;
      }
      ++ndist;
    } else if (cmd == "match") {
      int na = 0, nb = 0;
      uint64_t n = 0;
      in >> na >> nb >> n;
      std::vector<uint64_t> db((size_t)n);
      for (uint64_t& x : db) in >> x;
      if (!in || na < 1 || nb < 1 || n != (uint64_t)na * nb) throw std::runtime_error("malformed match case");
      std::vector<double> d(db.size());
      std::memcpy(d.data(), db.data(), db.size() * sizeof(double));
      if (!same_match(m.match_topics(d, na, nb), match_greedy(d.data(), na, nb))) {
        std::cerr << "model_compare_main: match case " << nmatch << " (" << na << " x " << nb << ") is not match_greedy's\n";
        return 3;
      }
      ++nmatch;
    } else {
      throw std::runtime_error("unknown case " + cmd);
    }
  }
  std::cout << ndist << " distance cases and " << nmatch << " matching cases equal match_host.h bit for bit\n";
  return 0;
}

int train(char** argv) {
  const word_id_t vocab_size = atol(argv[5]);
  const doc_id_t num_docs = atol(argv[6]);
  const doc_id_t num_topics = atol(argv[7]);
  ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[2], argv[3], argv[4]);
  trainer.train();
  trainer.output_cluster_summary();
  trainer.write_model_to_file();
  trainer.output_model_comparison(trainer.log_directory() + "/M_hat_catch_sparse", ISLE_TEXT_SPARSE);
  // the file against the statement of its bytes, on a second comparison of the same two resident models
  std::vector<double> dist;
  const FPSparseMatrixHip::TopicMatch again = trainer.matrix()->compare_models(ISLE_MODEL_CATCH, ISLE_MODEL_LOADED, &dist);
  const std::string want = trainer_detail::topic_match_text(again.match_a, again.match_dist);
  std::ifstream in(trainer.log_directory() + "/TopicMatch.tsv", std::ios::binary);
  const std::string got((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (got != want || got.empty()) {
    std::cerr << "model_compare_main: TopicMatch.tsv (" << got.size() << " bytes) is not topic_match_text's (" << want.size() << " bytes)\n";
    return 3;
  }
  // the matching against the host statement on the fetched models; the distances within the rule's bound of the plain loop's
  std::vector<FPTYPE> catch_model((size_t)vocab_size * num_topics), loaded;
  trainer.get_basic_model(catch_model.data());
  trainer.matrix()->get_loaded_model(loaded);
  std::vector<double> plain;
  model_dist_plain(catch_model.data(), (int)num_topics, loaded.data(), (int)num_topics, vocab_size, plain);
  const McMatch host = match_greedy(plain.data(), (int)num_topics, (int)num_topics);
  const double bound = 2.0 * 1.01 * (double)vocab_size * std::ldexp(1.0, -53);  // the device and the plain loop each within 1.01 V 2^-53 of the exact sum
  bool ok = again.match_a == host.match_a && again.match_b == host.match_b && again.n_matched == host.n_matched;
  for (size_t e = 0; ok && e < plain.size(); ++e)
    ok = std::isnan(plain[e]) ? std::isnan(dist[e]) : std::fabs(dist[e] - plain[e]) <= bound * plain[e];
  if (!ok) {
    std::cerr << "model_compare_main: the device's comparison of the catch model with the loaded file is not match_host.h's\n";
    return 3;
  }
  std::cout << "TopicMatch.tsv: " << got.size() << " bytes equal topic_match_text, " << again.n_matched << " of " << num_topics << " topics matched as match_greedy does\n";
  std::cout << "log directory: " << trainer.log_directory() << "\n";
  return 0;
}

int timed(char** argv) {
  const uint64_t V = strtoull(argv[2], nullptr, 10);
  const int ka = atoi(argv[3]), kb = atoi(argv[4]);
  uint64_t s = 12345;
  auto unit = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((s >> 40) / 16777216.0);
  };
  std::vector<float> a((size_t)V * ka), b((size_t)V * kb);
  for (float& x : a) x = unit();
  for (float& x : b) x = unit();
  FPSparseMatrixHip m(1, 1);
  double ms[5];
  for (int r = -1; r < 5; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    m.compare_models(ISLE_MODEL_HOST, ISLE_MODEL_HOST, nullptr, a.data(), ka, b.data(), kb, (word_id_t)V);
    if (r >= 0) ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  std::sort(ms, ms + 5);
  std::cout << "compare_models " << V << " words, " << ka << " x " << kb << ": median " << ms[2] << " ms, min " << ms[0] << ", max " << ms[4] << " (wall, uploads included)\n";
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc == 3 && std::string(argv[1]) == "check") return check(argv[2]);
    if (argc == 8 && std::string(argv[1]) == "train") return train(argv);
    if (argc == 5 && std::string(argv[1]) == "--time") return timed(argv);
    std::cerr << "usage: model_compare_main check <case_file> | train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> | --time <vocab_size> "
                 "<cols_a> <cols_b>\n";
    return 2;
  } catch (const std::exception& e) {
    std::cerr << "model_compare_main failed: " << e.what() << std::endl;
    return 1;
  }
}
