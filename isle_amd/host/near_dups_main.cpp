// isle_amd/host/near_dups_main.cpp — isle_hip_doc_signatures / isle_hip_doc_jaccard / isle_hip_doc_near_duplicates /
// isle_hip_prune_near_docs through FPSparseMatrixHip held to the plain loops of ../csrc/neardup_host.h, and ISLETrainer::prune_near_duplicates
// as a driver calls it (tests/test_gpu_near_dups_host_cpp.py).
//   near_dups_main check <vocab_size> <num_docs> <seed> <num> <den> <bands> <rows_per_band> <narrow> [--time]
//       a generated corpus (a Zipf-like head: word = V u^3; 5 .. 64 words a document; every fifth document a copy of an earlier one with
//       about a tenth of its words replaced, every eleventh an exact copy) is uploaded; signatures, band keys, the sizes of (document,
//       parent), parent, first_of, the three counters, kept_docs and the new A (offsets, rows, counts as their 32 bits) must equal what
//       nd_signatures_host / nd_keys_host / nd_jaccard_host / nd_rule / docs_prune_csc_host give: status 3 otherwise.  A refused shape must
//       be refused with the header's text.  --time: the median wall time of five device searches (doc_near_duplicates) and of five runs
//       of the host loops.
//   near_dups_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <num> <den> <bands> <rows_per_band>
//       FILE_DATA_LOAD, prune_near_duplicates, train, output_cluster_summary: DocsKept.tsv and NearDuplicates.tsv in the log directory,
//       whose name is printed.
#include <chrono>
#include <memory>

#include "trainer_hip.h"

#include "../csrc/neardup_host.h"

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

double median5(double* v) {
  std::sort(v, v + 5);
  return v[2];
}

int check(int argc, char** argv) {
  const uint64_t V = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10), seed = strtoull(argv[4], nullptr, 10);
  const uint64_t num = strtoull(argv[5], nullptr, 10), den = strtoull(argv[6], nullptr, 10);
  const int bands = atoi(argv[7]), rpb = atoi(argv[8]);
  const bool narrow = atoi(argv[9]) != 0;
  const bool timed = argc > 10 && std::string(argv[10]) == "--time";
  const int reps = timed ? 5 : 1;
  Lcg g = {seed * 2 + 1};
  std::vector<int64_t> offs(1, 0);
  std::vector<uint32_t> rows;
  std::vector<float> counts;
  const auto draw = [&]() {
    const double u = g.unit();
    return (uint32_t)std::min<double>((double)V - 1, (double)V * u * u * u);
  };
  for (uint64_t d = 0; d < D; ++d) {
    std::vector<uint32_t> words;
    if (d && (d % 5 == 4 || d % 11 == 10)) {  // a copy of an earlier document, near or exact
      const uint64_t from = g.next() % d;
      for (int64_t e = offs[from]; e < offs[from + 1]; ++e) words.push_back(d % 5 == 4 && g.next() % 10 == 0 ? draw() : rows[(size_t)e]);
    } else {
      const uint32_t len = 5 + g.next() % 60;
      for (uint32_t i = 0; i < len; ++i) words.push_back(draw());
    }
    std::sort(words.begin(), words.end());
    words.erase(std::unique(words.begin(), words.end()), words.end());
    for (uint32_t w : words) rows.push_back(w), counts.push_back((float)(1 + g.next() % 9));
    offs.push_back((int64_t)rows.size());
  }
  const uint64_t nnz = rows.size();
  std::vector<uint32_t> bits(nnz);
  if (nnz) std::memcpy(bits.data(), counts.data(), nnz * sizeof(uint32_t));

  // the plain loops
  const std::string refusal = nd_check_args("doc_near_duplicates", true, num, den, bands, rpb, 1);
  std::vector<uint64_t> sig_h, keys_h;
  std::vector<uint32_t> kept_h, cnt_h, rows_h;
  std::vector<int64_t> offs_h;
  NdResult want;
  double host_ms[5] = {0, 0, 0, 0, 0};
  if (refusal.empty()) {
    for (int rep = 0; rep < reps; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      nd_signatures_host(D, offs.data(), rows.data(), bands * rpb, sig_h);
      nd_keys_host(D, sig_h.data(), bands, rpb, keys_h);
      nd_rule(D, offs.data(), rows.data(), keys_h.data(), bands, narrow, num, den, want);
      host_ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    docs_prune_csc_host(D, offs.data(), bits.data(), rows.data(), want.keep.data(), 0, kept_h, offs_h, cnt_h, rows_h);
  }

  std::vector<doc_id_t> original_cols;
  std::unique_ptr<FPSparseMatrixHip> m(FPSparseMatrixHip::from_counts((word_id_t)V, (doc_id_t)D, counts.data(), rows.data(), offs.data(), 10, 0.0, original_cols));
  m->neardup_key_form(narrow ? ISLE_NEARDUP_KEY_NARROW : ISLE_NEARDUP_KEY_FULL);
  std::vector<uint32_t> parent, first_of, kept, inter, uni;
  uint64_t tested = 0, rounds = 0, dropped = 0;
  if (!refusal.empty()) {
    std::string got;
    try {
      m->near_duplicates(num, den, bands, rpb, parent, first_of);
    } catch (const std::exception& e) {
      got = e.what();
    }
    if (got != "doc_near_duplicates: " + refusal) {
      std::cerr << "near_dups_main: the device answers \"" << got << "\", the header \"" << refusal << "\"\n";
      return 3;
    }
    std::cout << "refused alike: " << refusal << "\n";
    return 0;
  }
  std::vector<uint64_t> sig_d, keys_d;
  m->doc_signatures(bands, rpb, &sig_d, &keys_d);
  double dev_ms[5] = {0, 0, 0, 0, 0};
  for (int rep = 0; rep < reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    dropped = m->near_duplicates(num, den, bands, rpb, parent, first_of, &tested, &rounds);
    dev_ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  const bool same_found = parent == want.parent && first_of == want.first_of && dropped == want.n_dropped && tested == want.pairs_tested && rounds == want.rounds;
  std::vector<uint32_t> p2, f2;
  uint64_t entries = 0;
  m->prune_near_duplicates(num, den, bands, rpb, kept, p2, f2, &inter, &uni, &entries);
  bool same_sizes = inter.size() == D && uni.size() == D;
  for (uint64_t d = 0; same_sizes && d < D; ++d) {
    uint32_t i = 0, u = 0;
    nd_jaccard_host(offs.data(), rows.data(), (uint32_t)d, want.parent[d], &i, &u);
    same_sizes = inter[d] == i && uni[d] == u;
  }
  std::vector<float> cnt_d;
  std::vector<uint32_t> rows_d;
  std::vector<int64_t> offs_d;
  m->get_count_matrix(cnt_d, rows_d, offs_d, nullptr);
  std::vector<uint32_t> bits_d(cnt_d.size());
  if (!cnt_d.empty()) std::memcpy(bits_d.data(), cnt_d.data(), cnt_d.size() * sizeof(uint32_t));
  const bool same_A = kept == kept_h && p2 == want.parent && f2 == want.first_of && entries == rows_h.size() && offs_d == offs_h && rows_d == rows_h && bits_d == cnt_h;
  if (sig_d != sig_h || keys_d != keys_h || !same_found || !same_sizes || !same_A) {
    std::cerr << "near_dups_main: the device result is not the plain loops' (signatures " << (sig_d == sig_h) << ", keys " << (keys_d == keys_h) << ", parent "
              << (parent == want.parent) << ", first_of " << (first_of == want.first_of) << ", dropped " << dropped << " / " << want.n_dropped << ", pairs tested "
              << tested << " / " << want.pairs_tested << ", rounds " << rounds << " / " << want.rounds << ", sizes " << same_sizes << ", kept_docs " << (kept == kept_h)
              << ", entries " << entries << " / " << rows_h.size() << ", offsets " << (offs_d == offs_h) << ", rows " << (rows_d == rows_h) << ", counts "
              << (bits_d == cnt_h) << ")\n";
    return 3;
  }
  std::cout << "documents " << D << " -> " << kept.size() << " (near duplicates " << dropped << ", pairs tested " << tested << ", rounds " << rounds << "), entries " << nnz
            << " -> " << entries << ": signatures, keys, sizes, parent, first_of, kept_docs and A equal the plain loops\n";
  if (timed)
    std::cout << "{\"documents\": " << D << ", \"entries\": " << nnz << ", \"device_near_duplicates_ms\": " << median5(dev_ms) << ", \"host_loops_ms\": " << median5(host_ms)
              << "}\n";
  return 0;
}

int train(char** argv) {
  const word_id_t vocab_size = atol(argv[5]);
  const doc_id_t num_docs = atol(argv[6]), num_topics = atol(argv[7]);
  ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[2], argv[3], argv[4]);
  trainer.prune_near_duplicates(strtoull(argv[8], nullptr, 10), strtoull(argv[9], nullptr, 10), atoi(argv[10]), atoi(argv[11]));
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
    if (mode == "train" && argc == 12) return train(argv);
  } catch (const std::exception& e) {
    std::cerr << "near_dups_main failed: " << e.what() << std::endl;
    return 1;
  }
  std::cerr << "usage: near_dups_main check <vocab_size> <num_docs> <seed> <num> <den> <bands> <rows_per_band> <narrow> [--time]\n"
               "       near_dups_main train <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <num> <den> <bands> <rows_per_band>\n";
  return 2;
}
