// isle_amd/host/doc_report_main.cpp — the trainer's per-document report files as a driver gets them, held to their host statements.
// Loads a tdf file (FILE_DATA_LOAD) into a trainer built with print_doctopic = true, trains, writes the cluster summary and the model
// files — write_model_to_file() then writes DocCatchword.tsv and DocTopicCatchwordSums.tsv into the log directory — and calls
// print_top_two_topics() (TopTwoTopicsPerDoc.txt).  Then it fetches what the files print (A, avg_doc_sz, the catchwords, the (document,
// topic) sums) and compares, byte for byte,
//   the three files and the device text of ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC (written to DocTopicCatchwordSums_by_doc.tsv)
// with the host loops of trainer_hip.h: trainer_detail::doc_catchword_text (the reference's merge walk), doc_topic_sums_text (its
// comparator, ties by document) and top_two_text over top_two_from_sums (the top-two rule applied to the fetched sums).  Exit status 0:
// all four agree.
//   doc_report_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> [--time]
// --time prints, per kind, one line "<kind> device_ms <wall of write_doc_report> host_ms <wall of the host loop on the fetched arrays>"
// (single runs; the fetch is not part of either).
#include "trainer_hip.h"

using namespace ISLE;

static std::string slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error("cannot open " + path);
  std::ostringstream o;
  o << in.rdbuf();
  return o.str();
}
static double ms_since(const std::chrono::high_resolution_clock::time_point& t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
}

int main(int argc, char** argv) {
  const bool timed = argc == 8 && std::string(argv[7]) == "--time";
  if (argc != 7 && !timed) {
    std::cerr << "usage: doc_report_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> [--time]\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3],
                        false, 100000, false, false, false, /*print_doctopic*/ true, true);
    trainer.train();
    trainer.output_cluster_summary();
    trainer.write_model_to_file();
    trainer.print_top_two_topics();
    const std::string dir = trainer.log_directory();
    FPSparseMatrixHip* M = trainer.matrix();

    // what the files print, on the host
    std::vector<FPTYPE> counts, nv, sum_val;
    std::vector<uint32_t> rows, sum_topic;
    std::vector<int64_t> offs, sum_offs;
    float avg_doc_sz = 0.f;
    M->get_count_matrix(counts, rows, offs, &avg_doc_sz);
    M->get_doc_topic_sums(sum_offs, sum_topic, sum_val);
    nv.resize(counts.size());
    for (doc_id_t d = 0; d < num_docs; ++d) {  // normalize_docs, src/sparseMatrix.cpp:136-167: avg_doc_sz * (count / the document's sum)
      float sum = 0.f;
      for (int64_t i = offs[d]; i < offs[d + 1]; ++i) sum += counts[i];
      for (int64_t i = offs[d]; i < offs[d + 1]; ++i) nv[i] = avg_doc_sz * (counts[i] / sum);
    }
    std::vector<uint32_t> catchword_words;
    for (doc_id_t t = 0; t < num_topics; ++t)
      for (word_id_t w : trainer.catchword_lists()[t]) catchword_words.push_back((uint32_t)w);
    std::sort(catchword_words.begin(), catchword_words.end());  // parallel_sort by word, src/trainer.cpp:884-885

    const char* kind[4] = {"catchwords", "topic_sums", "topic_sums_by_doc", "top_two"};
    const std::string file[4] = {dir + "/DocCatchword.tsv", dir + "/DocTopicCatchwordSums.tsv", dir + "/DocTopicCatchwordSums_by_doc.tsv",
                                 dir + "/TopTwoTopicsPerDoc.txt"};
    const int what[4] = {ISLE_DOCREPORT_CATCHWORDS, ISLE_DOCREPORT_TOPIC_SUMS, ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC, ISLE_DOCREPORT_TOP_TWO};
    int bad = 0;
    for (int i = 0; i < 4; ++i) {
      double dev_ms = 0.0;
      if (i == 2 || timed) {  // the trainer wrote the other three; timed: once more, on its own
        const auto t0 = std::chrono::high_resolution_clock::now();
        M->write_doc_report(file[i], what[i]);
        dev_ms = ms_since(t0);
      }
      const auto t0 = std::chrono::high_resolution_clock::now();
      std::string host;
      if (i == 0) {
        host = trainer_detail::doc_catchword_text(catchword_words, offs.data(), rows.data(), nv.data(), num_docs);
      } else if (i == 3) {
        std::vector<int32_t> top1, top2;
        trainer_detail::top_two_from_sums(sum_offs.data(), sum_topic.data(), sum_val.data(), num_docs, top1, top2);
        host = trainer_detail::top_two_text(top1.data(), top2.data(), num_docs);
      } else {
        host = trainer_detail::doc_topic_sums_text(sum_offs.data(), sum_topic.data(), sum_val.data(), num_docs, i == 2);
      }
      const double host_ms = ms_since(t0);
      const std::string dev = slurp(file[i]);
      const bool same = dev == host;
      std::cout << "doc_report " << kind[i] << ": " << dev.size() << " bytes on the device, " << host.size() << " on the host: "
                << (same ? "equal" : "DIFFERENT") << std::endl;
      if (timed) std::cout << kind[i] << " device_ms " << dev_ms << " host_ms " << host_ms << std::endl;
      if (!same) ++bad;
      if (host.empty()) {
        std::cerr << "doc_report_main: " << kind[i] << " is empty: the corpus checks nothing" << std::endl;
        ++bad;
      }
    }
    return bad ? 1 : 0;
  } catch (const std::exception& e) {
    std::cerr << "doc_report_main failed: " << e.what() << std::endl;
    return 1;
  }
}
