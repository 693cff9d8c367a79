// isle_amd/host/trainer_coherence_main.cpp — ISLE::ISLETrainer with the reference constructor's trailing flags: loads a tdf file
// (FILE_DATA_LOAD), trains, writes the cluster summary with compute_avg_coherence as given, and writes every topic's top words as
// "<topic> <word> <word> ..." lines (0-based ids, heaviest first) so that a test can recompute the coherence the log reports
// (tests/test_gpu_trainer_coherence.py).
//   trainer_coherence_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <compute_avg_coherence 0|1> <topwords_out>
#include "trainer_hip.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 9) {
    std::cerr << "usage: trainer_coherence_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <compute_avg_coherence 0|1> "
                 "<topwords_out>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  const bool coherence = atoi(argv[7]) != 0;
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3],
                        false, 100000, false, false, coherence, false, true);
    trainer.train();
    trainer.output_cluster_summary();
    std::ofstream out(argv[8]);
    for (doc_id_t t = 0; t < num_topics; ++t) {
      out << t;
      for (const auto& tw : trainer.top_words()[t]) out << " " << tw.first;
      out << "\n";
    }
  } catch (const std::exception& e) {
    std::cerr << "trainer_coherence_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
