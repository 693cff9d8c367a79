// isle_amd/host/vocab_prune_main.cpp — isle_hip_prune_vocab held to the plain loop of ../csrc/vocab_host.h, and ISLETrainer::prune_vocabulary
// as a driver calls it (tests/test_gpu_vocab_prune_host_cpp.py).
//   vocab_prune_main check <vocab_size> <num_docs> <seed> <min_df> <max_df> <keep_n> [--time]
//       a generated corpus (a Zipf-like head: word = V u^3; counts whole, fractional and above 2^24; every seventh document empty) is
//       uploaded, pruned on the device and fetched; df, kept_words, docs_emptied and the new A (offsets, rows, counts as their 32 bits) must
//       equal what vocab_df_host / vocab_rule / vocab_prune_csc_host give, bit for bit: status 3 otherwise.  --time: the median wall time of
//       three device prunes (each on a fresh upload, the upload not timed) and of three runs of the host loop.
//   vocab_prune_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <min_df> <max_df> <keep_n>
//       FILE_DATA_LOAD, prune_vocabulary, train, output_cluster_summary, output_top_words: VocabKept.tsv and TopWordsPerTopic_catch.txt
//       in the log directory, whose name is printed.
#include <chrono>

#include "trainer_hip.h"

#include "../csrc/vocab_host.h"

using namespace ISLE;

namespace {

struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  double unit() { return next() / 2147483648.0; }
};

void chk(isle_ctx* c, int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + isle_hip_last_error(c));
}

double median3(double a, double b, double c) { return std::max(std::min(a, b), std::min(std::max(a, b), c)); }

int check(int argc, char** argv) {
  const uint64_t V = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10), seed = strtoull(argv[4], nullptr, 10);
  const uint64_t min_df = strtoull(argv[5], nullptr, 10), max_df = strtoull(argv[6], nullptr, 10), keep_n = strtoull(argv[7], nullptr, 10);
  const bool timed = argc > 8 && std::string(argv[8]) == "--time";
  Lcg g = {seed * 2 + 1};
  std::vector<int64_t> offs(1, 0);
  std::vector<uint32_t> rows;
  std::vector<float> counts;
  for (uint64_t d = 0; d < D; ++d) {
    std::vector<uint32_t> words;
    if (d % 7 != 3) {
      const uint32_t len = 1 + g.next() % 60;
      for (uint32_t i = 0; i < len; ++i) {
        const double u = g.unit();
        words.push_back((uint32_t)std::min<double>((double)V - 1, (double)V * u * u * u));
      }
      std::sort(words.begin(), words.end());
      words.erase(std::unique(words.begin(), words.end()), words.end());
    }
    for (uint32_t w : words) {
      rows.push_back(w);
      const uint32_t kind = g.next() % 16;
      counts.push_back(kind == 0 ? 0.5f + (float)(g.next() % 7) : kind == 1 ? 16777217.0f + 2.0f * (float)(g.next() % 1000) : (float)(1 + g.next() % 9));
    }
    offs.push_back((int64_t)rows.size());
  }
  const uint64_t nnz = rows.size();
  std::vector<uint32_t> bits(nnz);
  if (nnz) std::memcpy(bits.data(), counts.data(), nnz * sizeof(uint32_t));

  // the plain loop
  std::vector<uint32_t> df_h, remap, kept_h, cnt_h, rows_h;
  std::vector<int64_t> offs_h;
  uint64_t emptied_h = 0;
  std::string refusal;
  double host_ms[3] = {0, 0, 0};
  for (int rep = 0; rep < (timed ? 3 : 1); ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    df_h.assign((size_t)V, 0);
    vocab_df_host(D, offs.data(), rows.data(), df_h.data());
    refusal = vocab_check_args(true, min_df, max_df, keep_n, D);
    if (refusal.empty()) refusal = vocab_rule(df_h.data(), V, min_df, max_df, keep_n, D, remap, kept_h);
    if (refusal.empty()) emptied_h = vocab_prune_csc_host(D, offs.data(), bits.data(), rows.data(), remap.data(), offs_h, cnt_h, rows_h);
    host_ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }

  isle_ctx* c = isle_hip_create(0);
  if (!c) throw std::runtime_error("isle_hip_create failed: no MI355X device (there is no CPU fallback)");
  int status = 0;
  try {
    std::vector<uint32_t> df_d((size_t)V), kept_d((size_t)V);
    uint64_t new_vocab = 0, nnz_d = 0, emptied_d = 0;
    double dev_ms[3] = {0, 0, 0};
    int rc = 0;
    for (int rep = 0; rep < (timed ? 3 : 1); ++rep) {
      chk(c, isle_hip_upload_counts_u32(c, V, D, nnz, counts.data(), rows.data(), offs.data(), 0, 0), "upload_counts");
      chk(c, isle_hip_synchronize(c), "synchronize");
      const auto t0 = std::chrono::steady_clock::now();
      rc = isle_hip_prune_vocab(c, min_df, max_df, keep_n, &new_vocab, kept_d.data(), df_d.data(), &nnz_d, &emptied_d);
      dev_ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rc != 0) break;
    }
    if (!refusal.empty() || rc != 0) {
      const std::string got = rc != 0 ? isle_hip_last_error(c) : "";
      if (rc != ISLE_E_ARG || got != refusal) {
        std::cerr << "vocab_prune_main: the device answers " << rc << " \"" << got << "\", the plain loop \"" << refusal << "\"\n";
        status = 3;
      } else {
        std::cout << "refused alike: " << got << "\n";
      }
    } else {
      std::vector<int64_t> offs_d((size_t)D + 1);
      std::vector<uint32_t> cnt_d((size_t)nnz_d), rows_d((size_t)nnz_d);
      chk(c, isle_hip_get_A(c, (float*)cnt_d.data(), rows_d.data(), offs_d.data()), "get_A");
      kept_d.resize((size_t)new_vocab);
      const bool same = df_d == df_h && kept_d == kept_h && emptied_d == emptied_h && nnz_d == rows_h.size() && offs_d == offs_h && rows_d == rows_h && cnt_d == cnt_h;
      if (!same) {
        std::cerr << "vocab_prune_main: the device result is not the plain loop's (df " << (df_d == df_h) << ", kept_words " << (kept_d == kept_h) << ", emptied "
                  << emptied_d << " / " << emptied_h << ", entries " << nnz_d << " / " << rows_h.size() << ", offsets " << (offs_d == offs_h) << ", rows "
                  << (rows_d == rows_h) << ", counts " << (cnt_d == cnt_h) << ")\n";
        status = 3;
      } else {
        std::cout << "V " << V << " -> " << new_vocab << ", entries " << nnz << " -> " << nnz_d << ", documents emptied " << emptied_d
                  << ": df, kept_words and A equal the plain loop bit for bit\n";
      }
    }
    if (timed && status == 0)
      std::cout << "{\"entries\": " << nnz << ", \"device_prune_ms\": " << median3(dev_ms[0], dev_ms[1], dev_ms[2]) << ", \"host_loop_ms\": "
                << median3(host_ms[0], host_ms[1], host_ms[2]) << "}\n";
  } catch (...) {
    isle_hip_destroy(c);
    throw;
  }
  isle_hip_destroy(c);
  return status;
}

int train(char** argv) {
  const word_id_t vocab_size = atol(argv[5]);
  const doc_id_t num_docs = atol(argv[6]), num_topics = atol(argv[7]);
  ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[2], argv[3], argv[4]);
  trainer.prune_vocabulary(strtoull(argv[8], nullptr, 10), strtoull(argv[9], nullptr, 10), strtoull(argv[10], nullptr, 10));
  trainer.train();
  trainer.output_cluster_summary();
  trainer.output_top_words();
  std::cout << "log directory: " << trainer.log_directory() << "\n";
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "check" && (argc == 8 || argc == 9)) return check(argc, argv);
    if (mode == "train" && argc == 11) return train(argv);
  } catch (const std::exception& e) {
    std::cerr << "vocab_prune_main failed: " << e.what() << std::endl;
    return 1;
  }
  std::cerr << "usage: vocab_prune_main check <vocab_size> <num_docs> <seed> <min_df> <max_df> <keep_n> [--time]\n"
               "       vocab_prune_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <min_df> <max_df> <keep_n>\n";
  return 2;
}
