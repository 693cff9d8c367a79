// isle_amd/host/docs_prune_main.cpp — isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs held to the plain loop of
// ../csrc/docs_host.h, and ISLETrainer::prune_documents as a driver calls it (tests/test_gpu_docs_prune_host_cpp.py).
//   docs_prune_main check <vocab_size> <num_docs> <seed> <min_words> <max_words> <min_tokens> <max_tokens> <drop_duplicates> [--time]
//       a generated corpus (a Zipf-like head: word = V u^3; counts whole, fractional and above 2^24; every seventh document empty, every
//       fifth a copy of an earlier one) is uploaded, pruned on the device and fetched; words, tokens, first_of over all documents, the
//       reported first_of, kept_docs, dropped and the new A (offsets, rows, counts as their 32 bits) must equal what docs_lengths_host /
//       docs_first_of_host / docs_rule / docs_prune_csc_host give, bit for bit: status 3 otherwise.  --time: the median wall time of five
//       device prunes (each on a fresh upload, the upload not timed) and of five runs of the host loop.
//   docs_prune_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <min_words> <max_words> <min_tokens>
//                         <max_tokens> <drop_duplicates>
//       FILE_DATA_LOAD, prune_documents, train, output_cluster_summary: DocsKept.tsv in the log directory, whose name is printed.
#include <chrono>

#include "trainer_hip.h"

#include "../csrc/docs_host.h"

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

double median5(double* v) {
  std::sort(v, v + 5);
  return v[2];
}

int check(int argc, char** argv) {
  const uint64_t V = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10), seed = strtoull(argv[4], nullptr, 10);
  const DocsBounds b = {strtoull(argv[5], nullptr, 10), strtoull(argv[6], nullptr, 10), strtoull(argv[7], nullptr, 10), strtoull(argv[8], nullptr, 10)};
  const int dups = atoi(argv[9]);
  const bool timed = argc > 10 && std::string(argv[10]) == "--time";
  const int reps = timed ? 5 : 1;
  Lcg g = {seed * 2 + 1};
  std::vector<int64_t> offs(1, 0);
  std::vector<uint32_t> rows;
  std::vector<float> counts;
  for (uint64_t d = 0; d < D; ++d) {
    if (d % 5 == 4) {  // a copy of an earlier document
      const uint64_t from = g.next() % d;
      for (int64_t e = offs[from]; e < offs[from + 1]; ++e) rows.push_back(rows[(size_t)e]), counts.push_back(counts[(size_t)e]);
    } else if (d % 7 != 3) {
      std::vector<uint32_t> words;
      const uint32_t len = 1 + g.next() % 60;
      for (uint32_t i = 0; i < len; ++i) {
        const double u = g.unit();
        words.push_back((uint32_t)std::min<double>((double)V - 1, (double)V * u * u * u));
      }
      std::sort(words.begin(), words.end());
      words.erase(std::unique(words.begin(), words.end()), words.end());
      for (uint32_t w : words) {
        rows.push_back(w);
        const uint32_t kind = g.next() % 16;
        counts.push_back(kind == 0 ? 0.5f + (float)(g.next() % 7) : kind == 1 ? 16777217.0f + 2.0f * (float)(g.next() % 1000) : (float)(1 + g.next() % 9));
      }
    }
    offs.push_back((int64_t)rows.size());
  }
  const uint64_t nnz = rows.size();
  std::vector<uint32_t> bits(nnz);
  if (nnz) std::memcpy(bits.data(), counts.data(), nnz * sizeof(uint32_t));

  // the plain loop
  std::vector<uint32_t> words_h, all_first_h, keep_h, first_h, kept_h, cnt_h, rows_h;
  std::vector<uint64_t> tokens_h;
  std::vector<int64_t> offs_h;
  uint64_t dropped_h[3] = {0, 0, 0}, dup_h = 0;
  std::string refusal;
  double host_ms[5] = {0, 0, 0, 0, 0};
  for (int rep = 0; rep < reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    refusal = docs_check_args("prune_docs", true, b, dups, 1);
    if (refusal.empty()) {
      if (!docs_rule(D, offs.data(), bits.data(), rows.data(), b, dups, keep_h, first_h, dropped_h)) refusal = docs_none_kept(b, dups);
      else docs_prune_csc_host(D, offs.data(), bits.data(), rows.data(), keep_h.data(), 0, kept_h, offs_h, cnt_h, rows_h);
    }
    host_ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  docs_lengths_host(D, offs.data(), bits.data(), words_h, tokens_h);
  dup_h = docs_first_of_host(D, offs.data(), bits.data(), rows.data(), all_first_h);

  isle_ctx* c = isle_hip_create(0);
  if (!c) throw std::runtime_error("isle_hip_create failed: no MI355X device (there is no CPU fallback)");
  int status = 0;
  try {
    std::vector<uint32_t> words_d((size_t)D), all_first_d((size_t)D), first_d((size_t)D), kept_d((size_t)D);
    std::vector<uint64_t> tokens_d((size_t)D);
    uint64_t new_docs = 0, nnz_d = 0, global_d = 0, dropped_d[3] = {0, 0, 0}, dup_d = 0;
    double dev_ms[5] = {0, 0, 0, 0, 0};
    int rc = 0;
    for (int rep = 0; rep < reps; ++rep) {
      chk(c, isle_hip_upload_counts_u32(c, V, D, nnz, counts.data(), rows.data(), offs.data(), 0, 0), "upload_counts");
      if (rep == 0) {
        chk(c, isle_hip_doc_lengths(c, words_d.data(), tokens_d.data()), "doc_lengths");
        chk(c, isle_hip_doc_duplicates(c, all_first_d.data(), &dup_d), "doc_duplicates");
        if (words_d != words_h || tokens_d != tokens_h || all_first_d != all_first_h || dup_d != dup_h) {
          std::cerr << "docs_prune_main: the device's lengths or first-of-its-kind table are not the plain loop's (words " << (words_d == words_h) << ", tokens "
                    << (tokens_d == tokens_h) << ", first_of " << (all_first_d == all_first_h) << ", duplicates " << dup_d << " / " << dup_h << ")\n";
          status = 3;
        }
      }
      chk(c, isle_hip_synchronize(c), "synchronize");
      const auto t0 = std::chrono::steady_clock::now();
      rc = isle_hip_prune_docs(c, b.min_words, b.max_words, b.min_tokens, b.max_tokens, dups, &new_docs, kept_d.data(), first_d.data(), &nnz_d, &global_d, dropped_d);
      dev_ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rc != 0) break;
    }
    if (status == 0 && (!refusal.empty() || rc != 0)) {
      const std::string got = rc != 0 ? isle_hip_last_error(c) : "";
      if (rc != ISLE_E_ARG || got != refusal) {
        std::cerr << "docs_prune_main: the device answers " << rc << " \"" << got << "\", the plain loop \"" << refusal << "\"\n";
        status = 3;
      } else {
        std::cout << "refused alike: " << got << "\n";
      }
    } else if (status == 0) {
      std::vector<int64_t> offs_d((size_t)new_docs + 1);
      std::vector<uint32_t> cnt_d((size_t)nnz_d), rows_d((size_t)nnz_d);
      chk(c, isle_hip_get_A(c, (float*)cnt_d.data(), rows_d.data(), offs_d.data()), "get_A");
      kept_d.resize((size_t)new_docs);
      const bool same_dropped = std::equal(dropped_d, dropped_d + 3, dropped_h);
      const bool same = kept_d == kept_h && first_d == first_h && same_dropped && global_d == kept_h.size() && nnz_d == rows_h.size() && offs_d == offs_h &&
                        rows_d == rows_h && cnt_d == cnt_h;
      if (!same) {
        std::cerr << "docs_prune_main: the device result is not the plain loop's (kept_docs " << (kept_d == kept_h) << ", first_of " << (first_d == first_h)
                  << ", dropped " << same_dropped << ", entries " << nnz_d << " / " << rows_h.size() << ", offsets " << (offs_d == offs_h) << ", rows "
                  << (rows_d == rows_h) << ", counts " << (cnt_d == cnt_h) << ")\n";
        status = 3;
      } else {
        std::cout << "documents " << D << " -> " << new_docs << " (too short " << dropped_d[0] << ", too long " << dropped_d[1] << ", duplicates " << dropped_d[2]
                  << "), entries " << nnz << " -> " << nnz_d << ": lengths, first_of, kept_docs and A equal the plain loop bit for bit\n";
      }
    }
    if (timed && status == 0)
      std::cout << "{\"documents\": " << D << ", \"entries\": " << nnz << ", \"device_prune_ms\": " << median5(dev_ms) << ", \"host_loop_ms\": " << median5(host_ms) << "}\n";
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
  trainer.prune_documents(strtoull(argv[8], nullptr, 10), strtoull(argv[9], nullptr, 10), strtoull(argv[10], nullptr, 10), strtoull(argv[11], nullptr, 10),
                          atoi(argv[12]) != 0);
  trainer.train();
  trainer.output_cluster_summary();
  std::cout << "log directory: " << trainer.log_directory() << "\n";
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "check" && (argc == 10 || argc == 11)) return check(argc, argv);
    if (mode == "train" && argc == 13) return train(argv);
  } catch (const std::exception& e) {
    std::cerr << "docs_prune_main failed: " << e.what() << std::endl;
    return 1;
  }
  std::cerr << "usage: docs_prune_main check <vocab_size> <num_docs> <seed> <min_words> <max_words> <min_tokens> <max_tokens> <drop_duplicates> [--time]\n"
               "       docs_prune_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <min_words> <max_words> <min_tokens> "
               "<max_tokens> <drop_duplicates>\n";
  return 2;
}
