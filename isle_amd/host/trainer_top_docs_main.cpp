// isle_amd/host/trainer_top_docs_main.cpp — ISLE::ISLETrainer::output_topic_top_docs as a driver calls it: loads a tdf file
// (FILE_DATA_LOAD), trains, calls output_topic_top_docs(n) (TopDocsPerTopic.tsv, selected on the device from the resident catchword sums),
// then fetches those sums (FPSparseMatrixHip::get_doc_topic_sums), applies the host statement of the rule to them (topdocs_select_host,
// ../csrc/topdocs_host.h) and writes the lines it gives to <out>, so that a test can hold the file to the statement byte for byte
// (tests/test_gpu_top_docs_host_cpp.py).  Ends with status 3 where the two texts differ.
//   trainer_top_docs_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <n> <out>
#include "trainer_hip.h"

#include "../csrc/topdocs_host.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 9) {
    std::cerr << "usage: trainer_top_docs_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <n> <out>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  const uint32_t n = (uint32_t)atol(argv[7]);
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3]);
    trainer.train();
    trainer.output_topic_top_docs((int)n);
    std::vector<int64_t> offs;
    std::vector<uint32_t> topic;
    std::vector<FPTYPE> val;
    trainer.matrix()->get_doc_topic_sums(offs, topic, val);
    std::vector<uint32_t> bits(val.size()), docs((size_t)num_topics * n), vbits((size_t)num_topics * n), counts(num_topics);
    std::vector<uint64_t> entries(num_topics);
    if (!val.empty()) std::memcpy(bits.data(), val.data(), val.size() * sizeof(uint32_t));
    topdocs_select_host((uint32_t)num_topics, n, 0, offs.size() - 1, offs.data(), topic.data(), bits.data(), docs.data(), vbits.data(), counts.data(),
                        entries.data());
    std::string want;
    char text[40];
    for (doc_id_t t = 0; t < num_topics; ++t)
      for (uint32_t i = 0; i < counts[t]; ++i) {
        float w;
        std::memcpy(&w, &vbits[(size_t)t * n + i], sizeof(w));
        want.append(text, trainer_detail::doc_line_text((uint64_t)docs[(size_t)t * n + i] + 1, (uint64_t)t + 1, w, text));
      }
    {
      std::ofstream out(argv[8], std::ios::binary);
      out << want;
    }
    std::ifstream in(trainer.log_directory() + "/TopDocsPerTopic.tsv", std::ios::binary);
    const std::string got((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (got != want) {
      std::cerr << "trainer_top_docs_main: TopDocsPerTopic.tsv (" << got.size() << " bytes) is not the host statement (" << want.size() << " bytes)\n";
      return 3;
    }
    std::cout << "TopDocsPerTopic.tsv: " << got.size() << " bytes equal the host statement\n";
  } catch (const std::exception& e) {
    std::cerr << "trainer_top_docs_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
