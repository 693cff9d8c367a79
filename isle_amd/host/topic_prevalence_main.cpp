// isle_amd/host/topic_prevalence_main.cpp — FPSparseMatrixHip::topic_prevalence and ISLE::ISLETrainer::output_topic_prevalence as a driver
// calls them: loads a tdf file (FILE_DATA_LOAD), trains, asks for the prevalence of every topic over the whole corpus and over num_groups
// groups of documents (document d in group d % num_groups, every 17th document in no group), with and without normalise, summed on the
// device from the resident catchword sums; fetches those sums (FPSparseMatrixHip::get_doc_topic_sums), applies the host statement of the
// rule to them (prevalence_host, ../csrc/prevalence_host.h) and holds the device's arrays to it, == on the integers and on the bits of the
// doubles; then output_topic_prevalence (TopicPrevalence.tsv), parsed again, is held to the arrays.  One line per check on stdout, "ok" or
// "FAILED" first; ends with status 3 where a check failed (tests/test_gpu_topic_prevalence_host_cpp.py).
//   topic_prevalence_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <num_groups>
#include "trainer_hip.h"

#include "../csrc/prevalence_host.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 8) {
    std::cerr << "usage: topic_prevalence_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> <num_groups>\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  const uint32_t G = (uint32_t)atol(argv[7]);
  int failed = 0;
  auto report = [&](bool ok, const std::string& what) {
    std::cout << (ok ? "ok " : "FAILED ") << what << "\n";
    if (!ok) ++failed;
  };
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3]);
    bool refused = false;
    try {
      trainer.output_topic_prevalence({}, 1, false);
    } catch (const std::runtime_error&) {
      refused = true;
    }
    report(refused, "output_topic_prevalence before train() is refused");
    trainer.train();
    std::vector<int64_t> offs;
    std::vector<uint32_t> topic;
    std::vector<FPTYPE> val;
    trainer.matrix()->get_doc_topic_sums(offs, topic, val);
    const uint64_t rows = offs.size() - 1;
    std::vector<uint32_t> groups(rows);
    for (uint64_t d = 0; d < rows; ++d) groups[d] = d % 17 == 16 ? ISLE_GROUP_NONE : (uint32_t)(d % G);
    const size_t k = (size_t)num_topics;
    FPSparseMatrixHip::TopicPrevalence kept;
    for (int labelled = 0; labelled <= 1; ++labelled)
      for (int normalise = 0; normalise <= 1; ++normalise) {
        const uint32_t ng = labelled ? G : 1u;
        const std::vector<uint32_t> lab = labelled ? groups : std::vector<uint32_t>();
        const FPSparseMatrixHip::TopicPrevalence got = trainer.matrix()->topic_prevalence(ISLE_TOPDOCS_SUMS, num_topics, lab, ng, normalise != 0);
        std::vector<uint64_t> docs(ng), count(ng * k), dominant(ng * k);
        std::vector<double> sum(ng * k);
        uint64_t none = 0;
        prevalence_host((uint32_t)num_topics, rows, offs.data(), topic.data(), val.data(), labelled ? groups.data() : nullptr, ng, normalise, docs.data(), &none,
                        count.data(), dominant.data(), sum.data());
        const bool same = got.docs == docs && got.count == count && got.dominant == dominant && got.unlabelled == none &&
                          std::memcmp(got.sum.data(), sum.data(), sum.size() * sizeof(double)) == 0;
        uint64_t entries = 0;
        for (const uint64_t x : count) entries += x;
        report(same, std::string("topic_prevalence (") + (labelled ? "labels" : "no labels") + (normalise ? ", normalise" : "") +
                         ") is the host statement bit for bit: " + std::to_string(ng) + " groups, " + std::to_string(entries) + " entries, " +
                         std::to_string(none) + " rows in no group");
        if (labelled && !normalise) kept = got;
      }
    trainer.output_topic_prevalence(groups, G, false);
    std::ifstream in(trainer.log_directory() + "/TopicPrevalence.tsv");
    uint64_t lines = 0, cells = 0;
    bool same = true, ascending = true;
    long long before = -1;
    unsigned long long g, t, docs, with_topic, dominant;
    std::string s_sum, s_mean;
    while (in >> g >> t >> docs >> with_topic >> dominant >> s_sum >> s_mean) {
      ++lines;
      if (g >= G || t < 1 || t > k) {
        same = false;
        break;
      }
      const size_t at = (size_t)g * k + (t - 1);
      const double sum = std::strtod(s_sum.c_str(), nullptr), mean = std::strtod(s_mean.c_str(), nullptr);  // %.17g round-trips a double
      const double want_mean = kept.sum[at] / (double)kept.docs[g];
      same = same && docs == kept.docs[g] && with_topic == kept.count[at] && with_topic > 0 && dominant == kept.dominant[at] &&
             std::memcmp(&sum, &kept.sum[at], sizeof(double)) == 0 && std::memcmp(&mean, &want_mean, sizeof(double)) == 0;
      ascending = ascending && (long long)at > before;
      before = (long long)at;
    }
    for (const uint64_t x : kept.count) cells += x > 0;
    report(same && ascending && lines == cells && lines > 0,
           "TopicPrevalence.tsv parsed again is the arrays: " + std::to_string(lines) + " lines for " + std::to_string(cells) + " cells with count > 0");
  } catch (const std::exception& e) {
    std::cerr << "topic_prevalence_main failed: " << e.what() << std::endl;
    return 1;
  }
  return failed ? 3 : 0;
}
