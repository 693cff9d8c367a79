// isle_amd/host/trainer_infer_main.cpp — ISLETrainer::output_doc_topic_weights as a driver calls it: loads a tdf file
// (FILE_DATA_LOAD), trains, writes the cluster summary and the model files, then infers the topic weights of every document under
// the resident catch model and writes DocTopicWeights.tsv into the log directory.  <out>.catch.f32 gets the catch model (vocab x
// topics, column-major float32), so that a test can repeat the inference under the same model (tests/test_gpu_infer_resident.py).
//   trainer_infer_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <out>
#include "trainer_hip.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 8) {
    std::cerr << "usage: trainer_infer_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <out>\n";
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
    trainer.write_model_to_file();
    trainer.output_doc_topic_weights();
    std::vector<FPTYPE> catch_model((size_t)vocab_size * num_topics);
    trainer.get_basic_model(catch_model.data());
    std::ofstream out(out_base + ".catch.f32", std::ios::binary);
    out.write((const char*)catch_model.data(), catch_model.size() * sizeof(FPTYPE));
  } catch (const std::exception& e) {
    std::cerr << "trainer_infer_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
