// isle_amd/host/trainer_avg_coherence_main.cpp — ISLE::ISLETrainer's model-quality methods as a driver calls them: loads a tdf file
// (FILE_DATA_LOAD), trains, writes the cluster summary and the model files; with the flag it then keeps copies of those outputs
// (<out>.before.<name>), calls output_avg_topic_coherence() and output_topic_diversity(), and writes the model files again, so that a
// test can check that the existing outputs keep every byte.  <out> gets the average model's selected top words as
// "<topic> <word> <word> ..." lines (0-based ids, heaviest first); <out>.avg.f32 and <out>.catch.f32 the two models (vocab x topics,
// column-major float32) (tests/test_gpu_trainer_avg_model.py).
//   trainer_avg_coherence_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <quality 0|1> <out>
#include "trainer_hip.h"

using namespace ISLE;

static void copy_file(const std::string& from, const std::string& to) {
  std::ifstream in(from, std::ios::binary);
  std::ofstream out(to, std::ios::binary);
  out << in.rdbuf();
}

static void write_floats(const std::string& path, const FPTYPE* p, size_t n) {
  std::ofstream out(path, std::ios::binary);
  out.write((const char*)p, n * sizeof(FPTYPE));
}

int main(int argc, char** argv) {
  if (argc != 9) {
    std::cerr << "usage: trainer_avg_coherence_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <quality 0|1> <out>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  const bool quality = atoi(argv[7]) != 0;
  const std::string out_base = argv[8];
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3]);
    trainer.train();
    trainer.output_cluster_summary();
    trainer.write_model_to_file();
    std::ofstream out(out_base);
    if (quality) {
      for (const char* name : {"M_hat_catch_sparse", "TopWordsPerTopic_catch.txt", "diagnosticLog.txt"})
        copy_file(trainer.log_directory() + "/" + name, out_base + ".before." + name);
      FPTYPE avg = 0;
      std::vector<FPTYPE> coherences;
      trainer.output_avg_topic_coherence(avg, coherences);
      trainer.output_topic_diversity();
      trainer.write_model_to_file();
      for (doc_id_t t = 0; t < num_topics; ++t) {
        out << t;
        for (const auto& tw : trainer.avg_top_words()[t]) out << " " << tw.first;
        out << "\n";
      }
      write_floats(out_base + ".avg.f32", trainer.avg_model().data(), trainer.avg_model().size());
    }
    std::vector<FPTYPE> catch_model((size_t)vocab_size * num_topics);
    trainer.get_basic_model(catch_model.data());
    write_floats(out_base + ".catch.f32", catch_model.data(), catch_model.size());
  } catch (const std::exception& e) {
    std::cerr << "trainer_avg_coherence_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
