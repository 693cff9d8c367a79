// isle_amd/host/trainer_objective_main.cpp — ISLE::ISLETrainer::output_kmeans_objective as a driver calls it: loads a tdf file
// (FILE_DATA_LOAD), trains, writes the cluster summary, keeps a copy of the log (<out>.before.diagnosticLog.txt), calls
// output_kmeans_objective() and writes the partition's sizes to <out> as "<topic> <size>" lines (0-based), so that a test can hold
// ClusterObjective.tsv to the partition and check that the log only grew (tests/test_gpu_objective_host_cpp.py).
//   trainer_objective_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <out>
#include "trainer_hip.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 8) {
    std::cerr << "usage: trainer_objective_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <out>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  const std::string out_base = argv[7];
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3]);
    trainer.train();
    trainer.output_cluster_summary();
    {
      std::ifstream in(trainer.log_directory() + "/diagnosticLog.txt", std::ios::binary);
      std::ofstream copy(out_base + ".before.diagnosticLog.txt", std::ios::binary);
      copy << in.rdbuf();
    }
    trainer.output_kmeans_objective();
    std::ofstream out(out_base);
    for (doc_id_t t = 0; t < num_topics; ++t) out << t << " " << trainer.partition()[t].size() << "\n";
  } catch (const std::exception& e) {
    std::cerr << "trainer_objective_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
