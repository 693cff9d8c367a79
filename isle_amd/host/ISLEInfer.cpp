// isle_amd/host/ISLEInfer.cpp — the reference's inference driver (drivers/ISLEInfer.cpp) over the C ABI of include/isle_hip.h.
//
//   ISLEInfer <sparse_model_file> <infer_file> <output_dir> <num_topics> <vocab_size> <min_doc_id_in_infer_file>
//             <max_doc_id_in_infer_file> <nnzs_in_infer_file> <nnzs_in_sparse_model_file> <iters>[0 for default]
//             <Lifschitz_constant_guess>[0 for default]
//
// Same argument list (11 arguments, usage + exit(-1) otherwise, drivers/ISLEInfer.cpp:11-20), same inputs
// (M_hat_catch_sparse as written by ISLETrain: "<topic>\t<word>\t<weight>", 1-based, src/infer.cpp:125-190; tdf documents),
// same outputs: per block of 1,000,000 documents a file top_topics_iters_<iters>_Lf_<Lf>_doc_<first>_to_<last> with
// "<doc>\t<topic>\t<weight>" for the (at most five) topics heavier than 1 / num_topics (:100-112), and the summary lines on
// stdout (:159-176).  Everything heavy runs on the device and stays there: the model file is parsed by isle_hip_load_model_text
// (isle_amd/csrc/model_load.hip; model_read.h states its rule for the host), the documents go up once as a count matrix and
// isle_hip_infer_resident(ISLE_MODEL_LOADED) runs over the whole range; include/isle_hip.h documents that path as bit-equal to
// isle_hip_infer.  The output files are formatted on the device as well (isle_hip_infer_text, isle_amd/csrc/infer_text.hip), one call
// per file with the file as the sink; trainer_detail::write_doc_topic_lines (trainer_hip.h) states their bytes for the host.  There is
// no CPU fallback.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/isle_hip.h"
#include "model_read.h"
#include "prestage.h"

namespace {

int text_to_file(const char* bytes, uint64_t n, void* fp) { return std::fwrite(bytes, 1, (size_t)n, (FILE*)fp) == (size_t)n ? 0 : 1; }

// the eleven positional arguments (drivers/ISLEInfer.cpp:11-33: this order is the interface)
struct InferArgs {
  std::string model_path, docs_path, out_dir;
  uint64_t topics = 0, vocab = 0, first_doc = 0, last_doc = 0, doc_entries = 0;
  int iterations = 0;
  float lipschitz = 0.f;
};

[[noreturn]] void usage() {
  // the reference's wording, as scripts may grep for it
  std::cout << "Incorrect usage of ISLEInfer. Use: \n"
            << "inferFromFile <sparse_model_file> <infer_file> <output_dir> "
            << "<num_topics> <vocab_size> <min_doc_id_in_infer_file> <max_doc_id_in_infer_file>"
            << "<nnzs_in_infer_file> <nnzs_in_sparse_model_file> "
            << "<iters>[0 for default]  "
            << "Lifschitz_constant_guess>[0 for default]" << std::endl;
  std::exit(-1);
}

InferArgs read_args(int argc, char** argv) {
  if (argc != 12) usage();
  InferArgs a;
  a.model_path = argv[1];
  a.docs_path = argv[2];
  a.out_dir = argv[3];
  a.topics = std::strtoull(argv[4], nullptr, 10);
  a.vocab = std::strtoull(argv[5], nullptr, 10);
  a.first_doc = std::strtoull(argv[6], nullptr, 10);
  a.last_doc = std::strtoull(argv[7], nullptr, 10);
  a.doc_entries = std::strtoull(argv[8], nullptr, 10);
  // argv[9], the model's entry count, is not needed: the model file is read to its end
  a.iterations = (int)std::strtol(argv[10], nullptr, 10);
  if (a.iterations == 0) a.iterations = 15;  // INFER_ITERS_DEFAULT, include/hyperparams.h:81
  a.lipschitz = std::strtof(argv[11], nullptr);
  if (a.lipschitz == 0.0f) a.lipschitz = 10.0f;  // INFER_LF_DEAFULT :82
  if (a.topics < 1 || a.vocab < 1 || a.last_doc < a.first_doc) throw std::runtime_error("bad <num_topics> / <vocab_size> / document range");
  return a;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    const InferArgs args = read_args(argc, argv);
    const std::string &sparse_model_file = args.model_path, &infer_file = args.docs_path, &output_dir = args.out_dir;
    const uint64_t num_topics = args.topics, vocab_size = args.vocab, doc_begin = args.first_doc, doc_end = args.last_doc;
    const uint64_t max_entries = args.doc_entries;
    const int iters = args.iterations;
    const float Lfguess = args.lipschitz;

    isle_ctx* ctx = isle_hip_create(0);
    if (!ctx) throw std::runtime_error("no HIP device (there is no CPU fallback)");
    auto check = [&](int rc) {
      if (rc == 0) return;
      const std::string msg = isle_hip_last_error(ctx);
      isle_hip_destroy(ctx);
      throw std::runtime_error(msg);
    };

    std::cout << "Loading sparse model file: " << sparse_model_file << std::endl;
    {
      const std::vector<char> text = ISLE::model_read::read_file(sparse_model_file);
      check(isle_hip_load_model_text(ctx, text.data(), text.size(), vocab_size, (int)num_topics, ISLE_TEXT_SPARSE, 1, nullptr));
    }

    std::cout << "Loading data from inference file: " << infer_file << std::endl;
    std::vector<ISLE::prestage::DocWordEntry> entries;
    ISLE::prestage::read_tdf(infer_file, max_entries, entries, vocab_size, doc_end);  // ids up to doc_end pass; build_A holds them to the range
    const uint64_t num_docs = doc_end - doc_begin;  // drivers/ISLEInfer.cpp:49 (the last id of the range is not a document of its own)
    for (auto& e : entries) {  // :58: entries[i].doc -= (doc_begin - 1), ids already 0-based here
      if (e.doc + 1 < doc_begin) throw std::runtime_error("document id below <min_doc_id_in_infer_file>");
      e.doc -= (doc_begin - 1);
    }
    ISLE::prestage::Csc A;
    float avg_doc_sz = 0.f;  // the context computes the same value from the resident counts (populate_CSC's rule)
    uint64_t nz_docs = 0;
    ISLE::prestage::build_A(entries, vocab_size, num_docs, A, &avg_doc_sz, &nz_docs);  // sort, de-duplicate, populate_CSC (:50-59)
    std::vector<uint32_t> rows32(A.rows.begin(), A.rows.end());
    check(isle_hip_upload_counts_u32(ctx, vocab_size, num_docs, A.vals.size(), A.vals.data(), rows32.data(), A.offs.data(), 0, num_docs));

    std::vector<float> llh(num_docs * 2);
    uint64_t nconverged = 0;
    std::cout << "Creating inference engine" << std::endl;
    check(isle_hip_infer_resident(ctx, ISLE_MODEL_LOADED, nullptr, vocab_size, (int)num_topics, 0, num_docs, iters, Lfguess, -1.0f, 0, nullptr, nullptr,
                                  llh.data(), &nconverged, nullptr));

    // the heaviest topics stay on the device and every file is formatted there (isle_hip_infer_text), the file as the sink
    const uint64_t block = 1000000;  // :66
    for (uint64_t b0 = 0; b0 < num_docs; b0 += block) {
      const uint64_t b1 = std::min(num_docs, b0 + block);
      const std::string name = output_dir + "/top_topics_iters_" + std::to_string(iters) + "_Lf_" + std::to_string(Lfguess) + "_doc_" +
                               std::to_string(doc_begin + b0) + "_to_" + std::to_string(doc_begin + b1);
      FILE* f = std::fopen(name.c_str(), "wb");
      if (!f) {
        isle_hip_destroy(ctx);
        throw std::runtime_error("cannot open " + name);
      }
      const int rc = isle_hip_infer_text(ctx, ISLE_DOCTEXT_TOP, b0, b1, doc_begin, text_to_file, f, nullptr, nullptr);
      std::fclose(f);
      check(rc);
    }
    isle_hip_destroy(ctx);
    std::cout << "Number of docs for which inference converged: " << nconverged << " (of " << num_docs << ")" << std::endl;
    float sum_first = 0.f, sum_second = 0.f;  // :165-171 (fp32 sums in document order)
    for (uint64_t d = 0; d < num_docs; ++d) {
      sum_first += llh[2 * d];
      sum_second += llh[2 * d + 1];
    }
    std::cout << "Avg LLH per document for converged docs: " << ((float)num_docs / nconverged) * sum_first / nconverged << std::endl;
    std::cout << "Avg LLH per word: " << sum_second / max_entries << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "ISLEInfer: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
