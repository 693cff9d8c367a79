// isle_amd/host/trainer_diagnostics_main.cpp — ISLE::ISLETrainer with the reference constructor's compute_log_combinatorial and
// compute_distinct_top_five_sets flags, in either ingest mode: FILE_DATA_LOAD reads the tdf file itself; ITERATIVE_DATA_LOAD gets the
// same file fed document by document (feed_data + finalize_data, as drivers/trainer_export.cpp does).  Then it trains, so that the log
// files hold the whole run (tests/test_gpu_trainer_corpus_stats.py).
//   trainer_diagnostics_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <log_combinatorial 0|1>
//                            <distinct_top_five_sets 0|1> <file|iterative>
#include <string>

#include "trainer_hip.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 10) {
    std::cerr << "usage: trainer_diagnostics_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> "
                 "<log_combinatorial 0|1> <distinct_top_five_sets 0|1> <file|iterative>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  const bool log_comb = atoi(argv[7]) != 0, top_five = atoi(argv[8]) != 0;
  const std::string mode = argv[9];
  if (mode != "file" && mode != "iterative") {
    std::cerr << "ingest mode must be file or iterative\n";
    return 2;
  }
  try {
    if (mode == "file") {
      ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2],
                          argv[3], false, 100000, log_comb, top_five);
      trainer.train();
    } else {
      std::vector<std::vector<std::pair<word_id_t, count_t>>> docs(num_docs);
      {
        std::ifstream in(argv[1]);
        uint64_t d, w, cnt;
        while (in >> d >> w >> cnt) docs.at(d - 1).push_back(std::make_pair((word_id_t)w, (count_t)cnt));  // 1-based ids; feed_data takes the word as it is
      }
      ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::ITERATIVE_DATA_LOAD, argv[1], argv[2],
                          argv[3], false, 100000, log_comb, top_five);
      for (doc_id_t d = 0; d < num_docs; ++d) {
        std::vector<word_id_t> words;
        std::vector<count_t> counts;
        for (const auto& e : docs[d]) {
          words.push_back(e.first);
          counts.push_back(e.second);
        }
        trainer.feed_data(d, words.data(), counts.data(), (offset_t)words.size());
      }
      trainer.finalize_data();
      trainer.train();
    }
  } catch (const std::exception& e) {
    std::cerr << "trainer_diagnostics_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
