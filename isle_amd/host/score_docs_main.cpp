// isle_amd/host/score_docs_main.cpp — FPSparseMatrixHip::score_documents and ISLE::ISLETrainer::output_doc_scores as a driver calls them:
// loads a tdf file (FILE_DATA_LOAD), trains, infers the weights of every document (output_doc_topic_weights), fetches the count matrix, the
// catch model and the weights, and holds the device to the host statement of the rule (score_docs_host, ../csrc/score_host.h): on the
// resident count matrix and on the held-out part of every document (score_held_out, seed 1, one entry in three), ISLE_SCORE_PROB without
// normalise == on the bits of every array; ISLE_SCORE_LOG with normalise == on tokens and the counters, two calls the same bits, and the
// scores within 1e-12 of the host loop's (the two logarithms differ).  Then output_doc_scores on the held-out part: DocScores.tsv is
// trainer_detail::doc_scores_text of the arrays, byte for byte.  One line per check on stdout, "ok" or "FAILED" first; ends with status 3
// where a check failed (tests/test_gpu_score_docs_host_cpp.py).  --time: one JSON line more, the wall of five score_documents calls on the
// resident matrix (median, min, max in ms; each call synchronises).
//   score_docs_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> [--time]
#include <chrono>

#include "trainer_hip.h"

#include "../csrc/score_host.h"

using namespace ISLE;

namespace {

struct Host {
  std::vector<double> score, tokens, ut;
  std::vector<uint32_t> ue, fl;
};

bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

}  // namespace

int main(int argc, char** argv) {
  const bool timed = argc == 8 && std::string(argv[7]) == "--time";
  if (argc != 7 && !timed) {
    std::cerr << "usage: score_docs_main <tdf_file> <vocab_file> <output_dir> <vocab_size> <num_docs> <num_topics> [--time]\n";
    return 2;
  }
  const word_id_t vocab_size = atol(argv[4]);
  const doc_id_t num_docs = atol(argv[5]);
  const doc_id_t num_topics = atol(argv[6]);
  int failed = 0;
  auto report = [&](bool ok, const std::string& what) {
    std::cout << (ok ? "ok " : "FAILED ") << what << "\n";
    if (!ok) ++failed;
  };
  try {
    ISLETrainer trainer(vocab_size, num_docs, 0, num_topics, false, false, 0.0f, ISLETrainer::data_ingest::FILE_DATA_LOAD, argv[1], argv[2], argv[3]);
    bool refused = false;
    try {
      trainer.output_doc_scores();
    } catch (const std::runtime_error&) {
      refused = true;
    }
    report(refused, "output_doc_scores before train() is refused");
    trainer.train();
    FPSparseMatrixHip* const A = trainer.matrix();
    const doc_id_t docs = A->count_docs();
    refused = false;
    try {
      A->score_documents(ISLE_MODEL_CATCH, 0, docs, ISLE_SCORE_LOG, true, 0.0);
    } catch (const std::runtime_error& e) {
      refused = std::string(e.what()).find("no resident result") != std::string::npos;
    }
    report(refused, "score_documents before an inference is refused");
    trainer.output_doc_topic_weights();
    std::vector<FPTYPE> cnt, model((size_t)vocab_size * num_topics);
    std::vector<uint32_t> rows;
    std::vector<int64_t> offs;
    A->get_count_matrix(cnt, rows, offs, nullptr);
    trainer.get_basic_model(model.data());
    std::vector<int64_t> w_off;
    std::vector<uint32_t> w_topic;
    std::vector<FPTYPE> w_weight;
    A->infer_documents(ISLE_MODEL_CATCH, 0, docs, ISLE_INFER_ITERS_DEFAULT, ISLE_INFER_LF_DEFAULT, w_off, w_topic, w_weight);  // the same inference: the same entries
    // the held-out part of every document
    std::vector<FPTYPE> h_cnt;
    std::vector<uint32_t> h_rows;
    std::vector<int64_t> h_offs(1, 0);
    for (doc_id_t d = 0; d < docs; ++d) {
      for (int64_t e = offs[d]; e < offs[d + 1]; ++e)
        if (score_held_out(1, d, rows[e], 1, 3)) {
          h_cnt.push_back(cnt[e]);
          h_rows.push_back(rows[e]);
        }
      h_offs.push_back((int64_t)h_rows.size());
    }
    const FPSparseMatrixHip::HeldEntries held = {h_cnt.data(), h_rows.data(), h_offs.data()};
    const double floor = 1e-12;
    for (int part = 0; part < 2; ++part) {
      const FPTYPE* const c = part ? h_cnt.data() : cnt.data();
      const uint32_t* const r = part ? h_rows.data() : rows.data();
      const int64_t* const o = part ? h_offs.data() : offs.data();
      const std::string name = part ? "the held-out third" : "the resident count matrix";
      for (int mode = 0; mode < 2; ++mode) {
        const int measure = mode ? ISLE_SCORE_LOG : ISLE_SCORE_PROB;
        const bool normalise = mode != 0;
        const double fl = mode ? floor : 0.0;
        const FPSparseMatrixHip::DocScores got = A->score_documents(ISLE_MODEL_CATCH, 0, docs, measure, normalise, fl, part ? &held : nullptr);
        Host h;
        h.score.resize(docs), h.tokens.resize(docs), h.ut.resize(docs), h.ue.resize(docs), h.fl.resize(docs);
        score_docs_host((uint32_t)num_topics, vocab_size, model.data(), docs, w_off.data(), w_topic.data(), w_weight.data(), c, r, o, measure, normalise ? 1 : 0, fl,
                        h.score.data(), h.tokens.data(), h.ue.data(), h.ut.data(), h.fl.data(), nullptr);
        bool ok = same_bits(got.tokens, h.tokens) && same_bits(got.unscored_tokens, h.ut) && got.unscored_entries == h.ue && got.floored == h.fl;
        uint64_t unscored = 0, floored = 0;
        for (doc_id_t d = 0; d < docs; ++d) unscored += h.ue[d], floored += h.fl[d];
        if (!mode) {
          ok = ok && same_bits(got.score, h.score);
          report(ok, "score_documents (prob) on " + name + " is the host statement bit for bit: " + std::to_string((long long)o[docs]) + " entries, " +
                         std::to_string(unscored) + " unscored");
        } else {
          const FPSparseMatrixHip::DocScores again = A->score_documents(ISLE_MODEL_CATCH, 0, docs, measure, normalise, fl, part ? &held : nullptr);
          ok = ok && same_bits(got.score, again.score) && got.total_score == again.total_score;
          for (doc_id_t d = 0; d < docs; ++d) ok = ok && std::fabs(got.score[d] - h.score[d]) <= 1e-12 * std::fabs(h.score[d]);
          ok = ok && got.total_tokens == score_total(h.tokens.data(), docs) && got.perplexity == std::exp(-got.total_score / got.total_tokens);
          report(ok, "score_documents (log, normalise) on " + name + ": counters and tokens bit for bit, two calls the same bits, scores within 1e-12: " +
                         std::to_string(floored) + " floored, perplexity " + std::to_string(got.perplexity));
        }
      }
    }
    trainer.output_doc_scores(&held, floor);
    const FPSparseMatrixHip::DocScores s = A->score_documents(ISLE_MODEL_CATCH, 0, docs, ISLE_SCORE_LOG, true, floor, &held);
    const std::string want = trainer_detail::doc_scores_text(1, s.tokens, s.score, s.unscored_entries);
    std::ifstream in(trainer.log_directory() + "/DocScores.tsv", std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    report(text == want && !text.empty(), "DocScores.tsv is the host loop's text byte for byte: " + std::to_string(text.size()) + " bytes, " + std::to_string(docs) + " lines");
    if (timed) {
      std::vector<double> ms;
      for (int i = 0; i < 6; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        A->score_documents(ISLE_MODEL_CATCH, 0, docs, ISLE_SCORE_LOG, true, floor);
        const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (i) ms.push_back(t);  // (the first call is the warm-up)
      }
      std::sort(ms.begin(), ms.end());
      std::printf("{\"what\": \"score_documents, resident, log, normalise\", \"docs\": %llu, \"entries\": %lld, \"wall_ms_median\": %.3f, \"wall_ms_min\": %.3f, "
                  "\"wall_ms_max\": %.3f}\n", (unsigned long long)docs, (long long)offs[docs], ms[2], ms.front(), ms.back());
    }
  } catch (const std::exception& e) {
    std::cerr << "score_docs_main failed: " << e.what() << std::endl;
    return 1;
  }
  return failed ? 3 : 0;
}
