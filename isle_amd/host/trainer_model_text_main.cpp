// isle_amd/host/trainer_model_text_main.cpp — the ISLETrain command's sequence on ISLE::ISLETrainer with edge topics on (train,
// output_cluster_summary, write_model_to_file, train_edge_topics, write_edgemodel_to_file), then output_avg_topic_coherence, and the three
// models behind the files it wrote as raw float32 (column-major): <dump>.catch.f32 (get_basic_model), <dump>.edge.f32 (get_edge_model,
// vocab x get_num_edge_topics; the count goes to <dump>.nedge) and <dump>.avg.f32, so that a test can hold M_hat_catch_sparse,
// EdgeModel_sparse and M_hat_avg against the text of exactly those floats (tests/test_gpu_trainer_model_text.py).
//   trainer_model_text_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <max_entries> <num_topics> <max_edge_topics> <dump>
#include "trainer_hip.h"

using namespace ISLE;

static void write_floats(const std::string& path, const FPTYPE* p, size_t n) {
  std::ofstream out(path, std::ios::binary);
  out.write((const char*)p, n * sizeof(FPTYPE));
}

int main(int argc, char** argv) {
  if (argc != 10) {
    std::cerr << "usage: trainer_model_text_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <max_entries> <num_topics> "
                 "<max_edge_topics> <dump>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const offset_t max_entries = atol(argv[6]);
  const doc_id_t num_topics = atol(argv[7]);
  const int max_edge_topics = atoi(argv[8]);
  const std::string dump = argv[9];
  try {
    ISLETrainer trainer(vocab_size, num_docs, max_entries, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2],
                        argv[3], true, max_edge_topics);
    trainer.train();
    trainer.output_cluster_summary();
    trainer.write_model_to_file();
    trainer.train_edge_topics();
    trainer.write_edgemodel_to_file();
    FPTYPE avg = 0;
    std::vector<FPTYPE> coherences;
    trainer.output_avg_topic_coherence(avg, coherences);
    trainer.finish_log();
    std::vector<FPTYPE> m((size_t)vocab_size * num_topics);
    trainer.get_basic_model(m.data());
    write_floats(dump + ".catch.f32", m.data(), m.size());
    const size_t ne = (size_t)trainer.get_num_edge_topics();
    std::vector<FPTYPE> e((size_t)vocab_size * ne);
    trainer.get_edge_model(e.data());
    write_floats(dump + ".edge.f32", e.data(), e.size());
    std::ofstream(dump + ".nedge") << ne << "\n";
    write_floats(dump + ".avg.f32", trainer.avg_model().data(), trainer.avg_model().size());
  } catch (const std::exception& e) {
    std::cerr << "trainer_model_text_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
