// isle_amd/host/trainer_hip.h — ISLE::ISLETrainer over the MI355X path: the reference's trainer class (include/trainer.h:97-265,
// src/trainer.cpp) with its constructor arguments, its data-ingest modes and the methods its drivers call —
//   ISLETrainer(...)  load_data_from_file()  feed_data()  finalize_data()  train()  output_cluster_summary()  write_model_to_file()
//   train_edge_topics()  write_edgemodel_to_file()  get_basic_model()  get_num_edge_topics()  get_edge_model()
// — so that drivers/ISLETrain.cpp (:34-46) and the stale export layer drivers/trainer_export.cpp (:31-98) read the same against it.
// What runs where: ingest, thresholding, the hot path of train() (src/trainer.cpp:490-571), catchwords, the topic model and the edge
// topics all run on the device through FPSparseMatrixHip (fpsparse_hip.h -> include/isle_hip.h); this class is the host-side order of
// calls, the log lines (diagnosticLog.txt / timerLog.txt with the reference's formats) and the output files.
// Topic coherence (compute_avg_coherence, off by default as in the reference): output_cluster_summary() scores the first
// DEFAULT_COHERENCE_NUM_WORDS top words of every topic on the device (FPSparseMatrixHip::topic_coherence) and prints the reference's
// commented-out "Coherence:" line per topic (:806), the real "Avg coherence:" (mean over topics with a finite value; a line counts the
// others) and flt_coh.  Deviations: flt_coh of a row is that row's topic's value (the reference indexes it by sorted position), raw_coh
// stays 0.  With the flag off every output byte is what it was without it.
// Corpus diagnostics (compute_log_combinatorial / compute_distinct_top_five_sets, off by default as in the reference): right after the
// data is in (both ingest modes), print_log_combinatorial() writes LogCombinatorial.txt and print_distinct_top_five_sets() prints the
// "Distinct top five sets:" line, both computed on the device from A (FPSparseMatrixHip, include/isle_hip.h for the deviations).
// Model quality (called by a driver after output_cluster_summary(); nothing in this class or the CLI calls them, as in the reference):
// output_avg_topic_coherence() builds the cluster-average model on the device (no catchwords), selects its 10 top words on the device,
// scores the first DEFAULT_COHERENCE_NUM_WORDS with topic_coherence, prints "Avg coherence without catchwords:" and writes M_hat_avg
// and TopWordsPerTopic_avg.txt; output_topic_diversity() prints the catch model's "Average topic diversity:".  Deviations: the
// reference scores empty top-word lists (every coherence 0, empty TopWordsPerTopic_avg.txt lines), uses topic 1's vector in every
// diversity cross term and accumulates in fp32; here the coherence is the mean over topics with a finite value (a line counts the
// others), the diversity is the stated formula in double, and M_hat_avg writes "nan" for the entries of an empty cluster.  raw_coh
// stays 0 (the reference's summary has that call commented out).
// Model files: M_hat_catch_sparse, EdgeModel_sparse and M_hat_avg are formatted on the device from the resident models
// (FPSparseMatrixHip::write_model_text / write_edge_model_text -> isle_hip_model_text / isle_hip_edge_topics_text) and streamed to the file;
// trainer_detail's host writers below define those bytes and are what the tests compare the device text against.  DocTopicWeights.tsv
// is formatted on the device in the same way (write_infer_text -> isle_hip_infer_text; trainer_detail::write_doc_topic_lines).
// Edge topics: train_edge_topics() selects the pairs on the device from the resident top-two topics (FPSparseMatrixHip::construct_edge_topics
// -> isle_hip_select_edge_pairs; the host rule fpsparse_detail::select_edge_pairs_host beyond ISLE_EDGE_TABLE_MAX_TOPICS topics) and writes
// the reference's two report files, EdgeTopicComposition.txt and EdgeTopicTopWords.txt (print_edge_topic_composition /
// print_edge_topic_top_words, src/trainer.cpp:1169-1245; trainer_detail::edge_composition_text / edge_top_words_text state their bytes),
// the edge topics' words selected on the device from the catch model's columns (isle_hip_edge_top_words).  No vocab x #edge matrix is
// kept on the host: get_edge_model() fetches it on first use.  Deviation: with fewer than 20 (10) words in the vocabulary the blocks
// print min(., vocab_size) entries; the reference reads out of range there.
// Per-document reports: output_doc_topic() writes DocCatchword.tsv and DocTopicCatchwordSums.tsv, print_top_two_topics() writes
// TopTwoTopicsPerDoc.txt (src/trainer.cpp:874-991, :1008-1040), all three formatted on the device from the resident catchword map, the
// (document, topic) sums and the top-two topics (FPSparseMatrixHip::write_doc_report -> isle_hip_doc_report_text); trainer_detail::
// doc_catchword_text / doc_topic_sums_text / top_two_text state their bytes.  With print_doctopic set, write_model_to_file() calls
// output_doc_topic() (the call the reference left commented out at :664-667); the flag defaults to false.  Deviation: equal (topic, value)
// pairs of DocTopicCatchwordSums.tsv go by document ascending (the reference's sort is unstable).
// Model comparison: output_model_comparison(model_file) reads a model file into the resident loaded model and compares this run's catch
// model with it on the device: L1 distances of all topic pairs in double, greedy matching (isle_amd/csrc/match_host.h states the rule; the
// optimal assignment is out of scope).  TopicMatch.tsv (trainer_detail::topic_match_text states its bytes) and the log line "Avg L1
// distance of matched topics:".  The reference has no such output; nothing in this class or the CLI calls it.
// Not mirrored (dead under the shipped hyper-parameters or outside the path): load_preprocessed_data_from_file,
// compute_input_svd, construct_edge_topics_v1.
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <ctime>
#include <fstream>
#include <iomanip>
#include <memory>
#include <numeric>
#include <sstream>

#include "fpsparse_hip.h"
#include "prestage.h"

namespace ISLE {
namespace trainer_detail {
struct Logs {
  std::ofstream diag, timer;
  clock_t u0;
  std::chrono::high_resolution_clock::time_point s0, sbegin;
  clock_t ubegin;
  explicit Logs(const std::string& dir) : diag(dir + "/diagnosticLog.txt"), timer(dir + "/timerLog.txt") {
    u0 = ubegin = std::clock();
    s0 = sbegin = std::chrono::high_resolution_clock::now();
  }
  void print(const std::string& s) {  // LogUtils::print_string: file + stdout
    diag << s << std::flush;
    std::cout << s << std::flush;
  }
  void next_time_secs(const std::string& text, int fill_len = 40) {  // include/timer.h:72-85
    const clock_t u1 = std::clock();
    const auto s1 = std::chrono::high_resolution_clock::now();
    std::ostringstream ostr;
    ostr << "Time for " << std::setfill('.') << std::setw(fill_len) << std::left << text << ((double)(u1 - u0)) / CLOCKS_PER_SEC
         << "s(user)  " << std::chrono::duration<double>(s1 - s0).count() << "s(sys)";
    std::cout << ostr.str() << std::endl;
    timer << ostr.str() << std::endl;
    u0 = u1;
    s0 = s1;
  }
  void total(const std::string& text) {  // include/timer.h:108-120
    std::ostringstream ostr;
    ostr << "Total time for " << std::setfill('.') << std::setw(50) << std::left << text
         << ((double)(std::clock() - ubegin)) / CLOCKS_PER_SEC << "s(user)  "
         << std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - sbegin).count() << "s(secs)";
    std::cout << ostr.str() << std::endl;
    timer << ostr.str() << std::endl;
  }
};

std::string log_dir_name(uint64_t num_topics, const std::string& base, bool sample_docs, float sample_rate, bool tf_idf) {  // src/utils.cpp:28-48
  std::string s = "log_t_" + std::to_string(num_topics) + "_eps1_" + std::to_string(1.0 / 60.0) + "_eps2_" + std::to_string(1.0 / 3.0) +
                  "_eps3_" + std::to_string(5.0) + "_kMppReps_" + std::to_string(1) + "_kMLowDReps_" + std::to_string(10) + "_kMReps_" +
                  std::to_string(10) + "_sample_" + std::to_string(sample_docs) + "_tfidf_" + std::to_string((int)tf_idf);
  if (sample_docs) s += "_Rate_" + std::to_string(sample_rate);
  return base + "/" + s;
}
// DenseMatrix::write_to_file_as_sparse (src/denseMatrix.cpp:155-186, mmap branch) with MMappedOutput::concat_int /
// concat_float (include/utils.h:405-478): "<topic>\t<word>\t<weight>\n", 1-based, entries <= 1e-8 skipped, the weight
// written as integer part, '.', then SIX digits produced by repeated multiplication in FPTYPE — truncated, not rounded
// (the before_dec / after_dec arguments of concat_float never reach ftoa_mv).
// The weight's text, exactly as the reference's writer emits it: the integer part in decimal (at most its six low digits), a point, then six
// fraction digits peeled off one at a time by multiplying the float remainder by ten (single precision, truncating).  Returns the length.
inline size_t weight_text(float w, char* out) {
  size_t len = 0;
  unsigned int whole = (unsigned int)w;
  char digits[8];
  int nd = 0;
  do {
    digits[nd++] = (char)('0' + whole % 10);
    whole /= 10;
  } while (whole > 0 && nd < 6);
  while (nd > 0) out[len++] = digits[--nd];
  out[len++] = '.';
  float rest = w - (float)((int)w);
  for (int place = 0; place < 6; ++place) {
    rest *= 10;
    const int digit = (int)rest;
    out[len++] = (char)('0' + digit);
    rest -= digit;
  }
  return len;
}
// DenseMatrix::write_to_file (src/denseMatrix.cpp:124-151, mmap branch) with concat_float -> ftoa_mv (include/utils.h:421-466): one
// topic per line, every entry followed by '\t', "0.0" for zero, otherwise weight_text's digits; "nan" for a NaN entry (an empty
// cluster; the reference's conversion of NaN to an integer is undefined).
inline size_t dense_entry_text(float w, char* out) {
  if (w != w) {
    std::memcpy(out, "nan", 3);
    return 3;
  }
  if (w == 0.0f) {
    std::memcpy(out, "0.0", 3);
    return 3;
  }
  return weight_text(w, out);
}
void write_dense(const std::string& filename, const float* M, uint64_t vocab_size, uint64_t ncols) {
  constexpr size_t kFlushAt = (size_t(1) << 24) - 256;
  FILE* fp = std::fopen(filename.c_str(), "wb");
  if (!fp) throw std::runtime_error("cannot open " + filename);
  std::string pending;
  pending.reserve(size_t(1) << 24);
  char text[32];
  for (uint64_t col = 0; col < ncols; ++col) {
    const float* column = M + col * vocab_size;
    for (uint64_t row = 0; row < vocab_size; ++row) {
      pending.append(text, dense_entry_text(column[row], text));
      pending += '\t';
      if (pending.size() > kFlushAt) {
        std::fwrite(pending.data(), 1, pending.size(), fp);
        pending.clear();
      }
    }
    pending += '\n';
  }
  std::fwrite(pending.data(), 1, pending.size(), fp);
  std::fclose(fp);
}
void write_dense_as_sparse(const std::string& filename, const float* M, uint64_t vocab_size, uint64_t ncols) {
  constexpr size_t kFlushAt = (size_t(1) << 24) - 256;
  FILE* fp = std::fopen(filename.c_str(), "wb");
  if (!fp) throw std::runtime_error("cannot open " + filename);
  std::string pending;
  pending.reserve(size_t(1) << 24);
  char text[32];
  for (uint64_t col = 0; col < ncols; ++col) {
    const float* column = M + col * vocab_size;
    for (uint64_t row = 0; row < vocab_size; ++row) {
      const float w = column[row];
      if (!(w > 0.00000001f)) continue;  // the reference skips entries at or below 1e-8
      pending += std::to_string(col + 1);
      pending += '\t';
      pending += std::to_string(row + 1);
      pending += '\t';
      pending.append(text, weight_text(w, text));
      pending += '\n';
      if (pending.size() > kFlushAt) {
        std::fwrite(pending.data(), 1, pending.size(), fp);
        pending.clear();
      }
    }
  }
  std::fwrite(pending.data(), 1, pending.size(), fp);
  std::fclose(fp);
}
// One line of the per-document topic files (ISLEInfer's top_topics_*, drivers/ISLEInfer.cpp:100-112; DocTopicWeights.tsv):
// "<doc>\t<topic>\t<weight>\n" with MMappedOutput::concat_int's plain decimals (include/utils.h:383-418) and weight_text's digits.
// doc_number and topic_number are the numbers as printed.  Returns the length (at most 36).
inline size_t doc_line_text(uint64_t doc_number, uint64_t topic_number, float w, char* out) {
  size_t len = 0;
  for (const uint64_t v : {doc_number, topic_number}) {
    const std::string digits = std::to_string(v);
    std::memcpy(out + len, digits.data(), digits.size());
    len += digits.size();
    out[len++] = '\t';
  }
  len += weight_text(w, out + len);
  out[len++] = '\n';
  return len;
}
// The two host loops the device formatter (isle_hip_infer_text) replaces, kept as the statement of its bytes: every entry of a CSR of
// document rows (offs: rows + 1; ISLE_DOCTEXT_ENTRIES), or with offs == nullptr the slots i = 0..4 of every row while topic[5 row + i] >= 0
// (ISLE_DOCTEXT_TOP).  Row r prints as r + number_base, a topic as topic + 1.
template <class TopicT>
void write_doc_topic_lines(FILE* fp, const int64_t* offs, const TopicT* topic, const float* weight, uint64_t rows, uint64_t number_base) {
  constexpr size_t kFlushAt = (size_t(1) << 24) - 256;
  std::string pending;
  pending.reserve(size_t(1) << 24);
  char text[40];
  auto put = [&](uint64_t row, int64_t at) {
    pending.append(text, doc_line_text(row + number_base, (uint64_t)topic[at] + 1, weight[at], text));
    if (pending.size() > kFlushAt) {
      std::fwrite(pending.data(), 1, pending.size(), fp);
      pending.clear();
    }
  };
  for (uint64_t row = 0; row < rows; ++row) {
    if (offs)
      for (int64_t i = offs[row]; i < offs[row + 1]; ++i) put(row, i);
    else
      for (int i = 0; i < 5 && topic[row * 5 + i] >= 0; ++i) put(row, (int64_t)(row * 5 + i));
  }
  std::fwrite(pending.data(), 1, pending.size(), fp);
}
// One line of TopTwoTopicsPerDoc.txt: three concat_int decimals, the numbers as printed.  Returns the length (at most 33).
inline size_t top_two_line_text(uint64_t doc_number, uint64_t t1_number, uint64_t t2_number, char* out) {
  size_t len = 0;
  const uint64_t v[3] = {doc_number, t1_number, t2_number};
  for (int i = 0; i < 3; ++i) {
    const std::string digits = std::to_string(v[i]);
    std::memcpy(out + len, digits.data(), digits.size());
    len += digits.size();
    out[len++] = i < 2 ? '\t' : '\n';
  }
  return len;
}
// The three host loops the device formatter (isle_hip_doc_report_text) replaces, kept as the statement of its bytes.  Everything is
// printed 1-based.
// DocCatchword.tsv (ISLETrainer::output_doc_topic, src/trainer.cpp:946-964): documents ascending; beside every column of A (rows
// ascending) the walk over the catchwords sorted by word, a line for every entry whose word is one.  catchword_words: ascending.
// nv: the normalised values of A (normalized_vals_CSC).
inline std::string doc_catchword_text(const std::vector<uint32_t>& catchword_words, const int64_t* offs, const uint32_t* rows, const float* nv,
                                      uint64_t docs) {
  std::string out;
  char text[40];
  for (uint64_t doc = 0; doc < docs; ++doc) {
    auto w_iter = catchword_words.begin();
    for (int64_t pos = offs[doc]; pos < offs[doc + 1]; ++pos) {
      while (w_iter != catchword_words.end() && *w_iter < rows[pos]) ++w_iter;
      if (w_iter == catchword_words.end()) continue;
      if (rows[pos] == *w_iter) out.append(text, doc_line_text(doc + 1, (uint64_t)*w_iter + 1, nv[pos], text));
    }
  }
  return out;
}
// DocTopicCatchwordSums.tsv (:979-983): the (document, topic, sum) triples (given as CSR over the documents, topics ascending) in the
// order construct_topic_model leaves them in (src/sparseMatrix.cpp:715-718): topic ascending, then value descending.  The reference's
// parallel_sort is unstable; here equal (topic, value) pairs go by document ascending (a stable sort of the (document, topic) order).
// by_doc: the resident order instead (ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC).
inline std::string doc_topic_sums_text(const int64_t* offs, const uint32_t* topic, const float* val, uint64_t docs, bool by_doc = false) {
  std::vector<std::tuple<uint64_t, uint32_t, float>> sums;
  for (uint64_t doc = 0; doc < docs; ++doc)
    for (int64_t i = offs[doc]; i < offs[doc + 1]; ++i) sums.emplace_back(doc, topic[i], val[i]);
  if (!by_doc)
    std::stable_sort(sums.begin(), sums.end(), [](const std::tuple<uint64_t, uint32_t, float>& l, const std::tuple<uint64_t, uint32_t, float>& r) {
      return std::get<1>(l) < std::get<1>(r) || (std::get<1>(l) == std::get<1>(r) && std::get<2>(l) > std::get<2>(r));
    });
  std::string out;
  char text[40];
  for (const auto& s : sums) out.append(text, doc_line_text(std::get<0>(s) + 1, (uint64_t)std::get<1>(s) + 1, std::get<2>(s), text));
  return out;
}
// The top-two topics of a document from its sums (src/sparseMatrix.cpp:687-708): -1 where it has fewer than two.
inline void top_two_from_sums(const int64_t* offs, const uint32_t* topic, const float* val, uint64_t docs, std::vector<int32_t>& top1,
                              std::vector<int32_t>& top2) {
  top1.assign(docs, -1);
  top2.assign(docs, -1);
  for (uint64_t doc = 0; doc < docs; ++doc) {
    float max = 0.0f, max2 = 0.0f;
    int max_topic = -1, max2_topic = -1;
    for (int64_t i = offs[doc]; i < offs[doc + 1]; ++i) {
      if (val[i] > max) {
        max2 = max;
        max2_topic = max_topic;
        max = val[i];
        max_topic = (int)topic[i];
      } else if (val[i] > max2) {
        max2 = val[i];
        max2_topic = (int)topic[i];
      }
    }
    top1[doc] = max_topic;
    top2[doc] = max2_topic;
  }
}
// TopTwoTopicsPerDoc.txt (ISLETrainer::print_top_two_topics, :1029-1035): documents ascending, those that have both topics.
inline std::string top_two_text(const int32_t* top1, const int32_t* top2, uint64_t docs) {
  std::string out;
  char text[40];
  for (uint64_t doc = 0; doc < docs; ++doc)
    if (top1[doc] >= 0 && top2[doc] >= 0) out.append(text, top_two_line_text(doc + 1, (uint64_t)top1[doc] + 1, (uint64_t)top2[doc] + 1, text));
  return out;
}
// The rule of ITERATIVE_DATA_LOAD on the host (src/trainer.cpp:232-371): the fed entries (zero counts already left out) sorted stably by
// (doc, word), the first fed of equal pairs kept, the CSC of A with its empty documents.  The trainer's data goes through the device feed
// (FPSparseMatrixHip::feed / from_feed -> isle_hip_feed_*), which is held to this statement by isle_amd/host/feed_main.cpp.
inline void csc_from_fed(doc_id_t num_docs, const std::vector<uint32_t>& fed_doc, const std::vector<uint32_t>& fed_word,
                         const std::vector<uint32_t>& fed_count, std::vector<float>& counts, std::vector<uint32_t>& rows, std::vector<offset_t>& offsets) {
  const size_t n = fed_doc.size();
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return fed_doc[a] < fed_doc[b] || (fed_doc[a] == fed_doc[b] && fed_word[a] < fed_word[b]);
  });
  counts.clear();
  rows.clear();
  offsets.assign((size_t)num_docs + 1, 0);
  counts.reserve(n);
  rows.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t e = order[i];
    if (i && fed_doc[e] == fed_doc[order[i - 1]] && fed_word[e] == fed_word[order[i - 1]]) continue;  // duplicate (doc, word): the first stays
    counts.push_back((float)fed_count[e]);
    rows.push_back(fed_word[e]);
    offsets[fed_doc[e] + 1]++;
  }
  for (doc_id_t d = 0; d < num_docs; ++d) offsets[d + 1] += offsets[d];
}
// EdgeTopicComposition.txt (print_edge_topic_composition, src/trainer.cpp:1169-1194): "<primary>\t<secondary>\t<documents>\n" per edge
// topic, topic ids 0-based as the reference prints them.
inline std::string edge_composition_text(const std::vector<std::tuple<int, int, uint64_t>>& pairs) {
  std::ostringstream o;
  for (const auto& p : pairs) o << std::get<0>(p) << '\t' << std::get<1>(p) << '\t' << std::get<2>(p) << '\n';
  return o.str();
}
// EdgeTopicTopWords.txt (print_edge_topic_top_words, src/trainer.cpp:1196-1245).  edge_ids / edge_w: n_edge_words top words per edge
// topic (row-major); topic_ids / topic_w: n_topic_words top words per BASIC topic (row-major, every topic); entries
// "word(id,weight)\t" with 0-based word ids and operator<< of the float.
inline std::string edge_top_words_text(const std::vector<std::tuple<int, int, uint64_t>>& pairs, const std::vector<std::string>& vocab_words,
                                       const uint32_t* edge_ids, const float* edge_w, const size_t n_edge_words, const uint32_t* topic_ids,
                                       const float* topic_w, const size_t n_topic_words) {
  std::ostringstream o;
  auto entries = [&](const uint32_t* ids, const float* w, size_t n) {
    for (size_t i = 0; i < n; ++i) o << vocab_words[ids[i]] << "(" << ids[i] << "," << w[i] << ")\t";
  };
  for (size_t t = 0; t < pairs.size(); ++t) {
    const int p = std::get<0>(pairs[t]), q = std::get<1>(pairs[t]);
    o << "Edge Topic: " << t << "  (" << p << ", " << q << "): " << std::get<2>(pairs[t]) << '\n';
    o << "Top words in edge_topic: \n";
    entries(edge_ids + t * n_edge_words, edge_w + t * n_edge_words, n_edge_words);
    o << "\n";
    o << "Top words in topic: " << p << "\n";
    entries(topic_ids + (size_t)p * n_topic_words, topic_w + (size_t)p * n_topic_words, n_topic_words);
    o << "\n";
    o << "Top words in topic: " << q << "\n";
    entries(topic_ids + (size_t)q * n_topic_words, topic_w + (size_t)q * n_topic_words, n_topic_words);
    o << "\n\n";
  }
  return o.str();
}
// TopicMatch.tsv (ISLETrainer::output_model_comparison): "<topic>\t<matched topic or -1>\t<distance>\n" per topic of this run, topics 1-based
// like the model files, the distance as %.17g and "nan" where the topic stayed unmatched.
inline std::string topic_match_text(const std::vector<int32_t>& match_a, const std::vector<double>& match_dist) {
  std::string out;
  char line[96];
  for (size_t t = 0; t < match_a.size(); ++t) {
    if (match_a[t] < 0) std::snprintf(line, sizeof line, "%llu\t-1\tnan\n", (unsigned long long)t + 1);
    else std::snprintf(line, sizeof line, "%llu\t%d\t%.17g\n", (unsigned long long)t + 1, match_a[t] + 1, match_dist[t]);
    out += line;
  }
  return out;
}
// DocScores.tsv (ISLETrainer::output_doc_scores): "<document>\t<tokens>\t<score>\t<unscored entries>\n" per document, documents 1-based from
// first_number, tokens and score as %.17g (a double read back is the same bits).
inline std::string doc_scores_text(const uint64_t first_number, const std::vector<double>& tokens, const std::vector<double>& score,
                                   const std::vector<uint32_t>& unscored_entries) {
  std::string out;
  char line[128];
  for (size_t d = 0; d < score.size(); ++d) {
    std::snprintf(line, sizeof line, "%llu\t%.17g\t%.17g\t%u\n", (unsigned long long)(first_number + d), tokens[d], score[d], unscored_entries[d]);
    out += line;
  }
  return out;
}
}  // namespace trainer_detail

class ISLETrainer {
 public:
  enum data_ingest { FILE_DATA_LOAD, PREPROCESSED_DATA_LOAD, ITERATIVE_DATA_LOAD };  // include/trainer.h:91-94

 private:
  word_id_t vocab_size;  // the constructor's, until prune_vocabulary() (the only writer)
  doc_id_t num_docs;  // the constructor's, until prune_documents() (the only other writer)
  const offset_t max_entries;
  const doc_id_t num_topics;
  const bool flag_tf_idf;  // a no-op in the reference too; only the directory name differs
  const bool flag_sample_docs;
  const FPTYPE sample_rate;
  const data_ingest how_data_loaded;
  const std::string input_file, vocab_file, output_path_base;
  const bool flag_construct_edge_topics;
  const int max_edge_topics;
  const bool flag_compute_log_combinatorial, flag_compute_distinct_top_five_sets;
  const bool flag_compute_avg_coherence, flag_print_doctopic, flag_print_top_two_topics;
  std::string log_dir;
  std::unique_ptr<trainer_detail::Logs> log;

  bool is_data_loaded = false, is_training_complete = false;
  // ITERATIVE_DATA_LOAD: the (doc, word, count) triples not yet on the device (src/trainer.cpp:200-230 keeps every DocWordEntry on the
  // host); at most kFeedStage of them, whatever the corpus: a full buffer goes to the device feed (flush_fed)
  enum : size_t { kFeedStage = size_t(4) << 20 };  // entries
  std::vector<uint32_t> fed_doc, fed_word, fed_count;
  bool feed_failed = false;  // the device feed was lost with batches in it: no later call may start a fresh one from the remainder
  void flush_fed() {
    if (feed_failed) throw std::runtime_error("the device feed failed earlier: the data fed so far is lost, build a new trainer");
    if (!B_fl_CSC) {
      B_fl_CSC = FPSparseMatrixHip::begin_feed(vocab_size, num_docs, (uint64_t)std::max<offset_t>(max_entries, 0));
      const size_t stage = std::min<size_t>(kFeedStage, max_entries > 0 ? (size_t)max_entries : kFeedStage);
      fed_doc.reserve(stage);
      fed_word.reserve(stage);
      fed_count.reserve(stage);
    }
    if (fed_doc.empty()) return;
    try {
      B_fl_CSC->feed(fed_doc.size(), fed_doc.data(), fed_word.data(), fed_count.data());
    } catch (...) {  // (ids were checked as they came in: this is the device failing)
      delete B_fl_CSC;
      B_fl_CSC = nullptr;
      feed_failed = true;
      std::vector<uint32_t>().swap(fed_doc);
      std::vector<uint32_t>().swap(fed_word);
      std::vector<uint32_t>().swap(fed_count);
      throw;
    }
    fed_doc.clear();
    fed_word.clear();
    fed_count.clear();
  }

  FPSparseMatrixHip* B_fl_CSC = nullptr;  // owns the device context: A (counts), B and everything derived from them live there
  std::vector<doc_id_t> original_cols;
  uint64_t entries_in_A = 0, entries_above_threshold = 0;
  float avg_doc_sz = 0.f;
  std::vector<FPTYPE> evalues;
  std::vector<doc_id_t>* closest_docs = nullptr;
  std::vector<word_id_t>* catchwords = nullptr;
  FPTYPE* catchword_thresholds = nullptr;
  FPTYPE* Model = nullptr;  // vocab_size x num_topics, column-major (DenseMatrix<FPTYPE>, include/denseMatrix.h:50-58)
  std::vector<std::tuple<int, int, doc_id_t>> top_topic_pairs;
  std::vector<std::tuple<int, int, uint64_t>> selected_pairs;
  std::vector<FPTYPE> EdgeModel;  // fetched by get_edge_model()
  bool edge_model_fetched = false;
  std::vector<std::string> vocab_words;
  word_id_t vocab_file_words = 0;     // prune_vocabulary(): the vocabulary the file's lines name (the constructor's vocab_size) ...
  std::vector<uint32_t> kept_words;   // ... and the line of every word of the current vocabulary; empty: never pruned
  std::vector<uint32_t> kept_docs;    // prune_documents(): the number every current document had when the data was loaded; empty: never pruned
  std::vector<std::vector<std::pair<word_id_t, FPTYPE>>> topwords;
  std::vector<std::vector<std::pair<word_id_t, FPTYPE>>> avg_topwords;  // output_avg_topic_coherence()
  std::vector<FPTYPE> AvgModel;  // vocab_size x num_topics, column-major, output_avg_topic_coherence()

  void print_header() {  // src/trainer.cpp:130-143
    std::ostringstream s;
    s << "\n<<<<<<<<<<<<\t" << input_file << "\t>>>>>>>>>>>>\n\n"
      << std::setfill('.') << std::setw(10) << std::left << std::setw(15) << std::left << "#Entries" << max_entries << "\n"
      << std::setw(15) << std::left << "#Words" << vocab_size << "\n"
      << std::setw(15) << std::left << "#Docs" << num_docs << "\n"
      << std::setw(15) << std::left << "#Topics" << num_topics << "\n"
      << std::setw(15) << std::left << "TF-IDF" << flag_tf_idf << "\n"
      << std::setw(15) << std::left << "Sampling?" << flag_sample_docs << "\n"
      << std::setw(15) << std::left << "Sample rate" << sample_rate << "\n"
      << std::setw(15) << std::left << "Edge topics?" << flag_construct_edge_topics << "\n"
      << std::setw(15) << std::left << "#Edge topics" << max_edge_topics << std::endl;
    log->print(s.str());
  }
  void print_log_combinatorial() {  // src/trainer.cpp:373-383
    std::vector<FPTYPE> docsLogFact;
    B_fl_CSC->compute_log_combinatorial(docsLogFact);
    std::ofstream out_comb_log(log_dir + "/LogCombinatorial.txt");
    for (auto iter = docsLogFact.begin(); iter != docsLogFact.end(); ++iter) out_comb_log << *iter << std::endl;
    out_comb_log.close();
    log->next_time_secs("Print Log Combinatorial");
  }
  void print_distinct_top_five_sets() {  // src/trainer.cpp:389-403
    std::ostringstream ostr;
    ostr << "Distinct top five sets: ";
    for (int m : {2, 5, 10, 20, 50, 100, 200, 500}) ostr << B_fl_CSC->count_distint_top_five_words(m) << " ";
    ostr << std::endl;
    log->print(ostr.str());
    log->next_time_secs("Distinct top-5 words");
  }
  void after_matrices_built() {  // the log lines of finalize_data / the thresholding block of train() (src/trainer.cpp:236-371, :430-485)
    log->next_time_secs("Sorting entries");
    log->next_time_secs("De-duplicating entries");
    std::cout << "Entries in sparse matrix: " << entries_in_A << std::endl << "Average document size: " << avg_doc_sz << std::endl;
    log->next_time_secs("Populating CSC");
    if (flag_compute_log_combinatorial) print_log_combinatorial();  // the end of load_data_from_file / finalize_data (:148-149, :210-211)
    if (flag_compute_distinct_top_five_sets) print_distinct_top_five_sets();
    log->next_time_secs("Computing thresholds");
    log->print("Number of entries above threshold: " + std::to_string(entries_above_threshold) + "\n");
    std::cout << (flag_sample_docs ? "After sampling docs: cols remaining: " : "Columns remaining after thresholding: ") << B_fl_CSC->num_docs() << "\n";
    log->next_time_secs("Creating thresholded and scaled matrix");
    is_data_loaded = true;
  }

 public:
  ISLETrainer(const word_id_t vocab_size_, const doc_id_t num_docs_, const offset_t max_entries_, const doc_id_t num_topics_, const bool tf_idf_,
              const bool sample_docs_, const FPTYPE sample_rate_, const data_ingest how_data_loaded_, const std::string& input_file_ = std::string(""),
              const std::string& vocab_file_ = std::string(""), const std::string& output_path_base_ = std::string(""),
              const bool construct_edge_topics_ = false, const int max_edge_topics_ = 100000, const bool compute_log_combinatorial_ = false,
              const bool compute_distinct_top_five_sets_ = false, const bool compute_avg_coherence_ = false, const bool print_doctopic_ = false,
              const bool print_top_two_topics_ = true)
      : vocab_size(vocab_size_), num_docs(num_docs_), max_entries(max_entries_), num_topics(num_topics_), flag_tf_idf(tf_idf_),
        flag_sample_docs(sample_docs_), sample_rate(sample_rate_), how_data_loaded(how_data_loaded_), input_file(input_file_),
        vocab_file(vocab_file_), output_path_base(output_path_base_), flag_construct_edge_topics(construct_edge_topics_),
        max_edge_topics(max_edge_topics_), flag_compute_log_combinatorial(compute_log_combinatorial_),
        flag_compute_distinct_top_five_sets(compute_distinct_top_five_sets_), flag_compute_avg_coherence(compute_avg_coherence_),
        flag_print_doctopic(print_doctopic_), flag_print_top_two_topics(print_top_two_topics_) {
    // src/trainer.cpp:8-81: log directory, the two log files, then the data according to the ingest mode
    log_dir = trainer_detail::log_dir_name(num_topics, output_path_base, flag_sample_docs, sample_rate, flag_tf_idf);
    struct stat st;
    if (stat(log_dir.c_str(), &st) == -1) mkdir(log_dir.c_str(), S_IRWXU);
    else std::cerr << "Subdir exists already" << std::endl;
    log.reset(new trainer_detail::Logs(log_dir));
    if (how_data_loaded == FILE_DATA_LOAD) load_data_from_file();
    else if (how_data_loaded == PREPROCESSED_DATA_LOAD) throw std::runtime_error("PREPROCESSED_DATA_LOAD is not mirrored (binary A_sp dumps of the reference)");
  }
  ~ISLETrainer() {
    delete[] closest_docs;
    delete[] catchwords;
    delete[] catchword_thresholds;
    delete[] Model;
    delete B_fl_CSC;
  }
  ISLETrainer(const ISLETrainer&) = delete;

  // src/trainer.cpp:124-150 + finalize_data :232-371 + the thresholding block of train() :430-485: tdf text -> A -> B, all on the device
  // (include/utils.h:96-229 for the format)
  void load_data_from_file() {
    FILE* f = std::fopen(input_file.c_str(), "rb");  // (a file that is not there is reported before any log line, as ever)
    if (!f) throw std::runtime_error("cannot open tdf file " + input_file);
    std::fclose(f);
    print_header();
    log->next_time_secs("Reading file Entries");
    // the file is streamed to the device in pieces, never held whole here or there (profiles/tdf_stream_c2.jsonl: 115 ms against 551 ms for the file read whole and ingested, config 2)
    B_fl_CSC = FPSparseMatrixHip::from_tdf_file(vocab_size, num_docs, input_file, max_entries, num_topics, flag_sample_docs ? (double)sample_rate : 0.0,
                                                original_cols, &entries_in_A, &entries_above_threshold, &avg_doc_sz);
    after_matrices_built();
  }

  // include/trainer.h:139-143, src/trainer.cpp:214-230: one document's words and counts.  The reference's convention, kept: `doc` is the
  // 0-based column, `words[i]` are 1-BASED word ids as in a tdf file (it stores `words[w] - 1`, :224).  Where the reference would write
  // outside its matrix, an id out of range is an error here.
  inline void feed_data(const doc_id_t doc, const word_id_t* const words, const count_t* const counts, const offset_t num_words) {
    if (how_data_loaded != ITERATIVE_DATA_LOAD) throw std::runtime_error("feed_data needs ITERATIVE_DATA_LOAD");
    if (is_data_loaded) throw std::runtime_error("feed_data after finalize_data");
    if (!B_fl_CSC || feed_failed) flush_fed();  // the first call opens the device feed, with room for max_entries; after a lost feed: throws
    for (offset_t i = 0; i < num_words; ++i) {
      if (doc >= num_docs || words[i] < 1 || words[i] > vocab_size) throw std::runtime_error("feed_data: id out of range (documents 0-based, words 1-based)");
      if (counts[i] == 0) continue;
      fed_doc.push_back((uint32_t)doc);
      fed_word.push_back((uint32_t)(words[i] - 1));
      fed_count.push_back((uint32_t)counts[i]);
      if (fed_doc.size() >= kFeedStage) flush_fed();
    }
  }
  // src/trainer.cpp:232-371: sort by (doc, word), keep the first of equal pairs, CSC of A — on the device, from the batches fed so far
  // (trainer_detail::csc_from_fed states the rule); then B is built there
  void finalize_data() {
    if (how_data_loaded != ITERATIVE_DATA_LOAD) throw std::runtime_error("finalize_data needs ITERATIVE_DATA_LOAD");
    if (is_data_loaded) throw std::runtime_error("finalize_data called twice");
    print_header();
    log->next_time_secs("Reading file Entries");
    flush_fed();
    std::vector<uint32_t>().swap(fed_doc);
    std::vector<uint32_t>().swap(fed_word);
    std::vector<uint32_t>().swap(fed_count);
    FPSparseMatrixHip* fed = B_fl_CSC;
    B_fl_CSC = nullptr;  // from_feed deletes it when it throws
    feed_failed = true;  // ... and the fed data is gone with it
    B_fl_CSC = FPSparseMatrixHip::from_feed(fed, num_topics, flag_sample_docs ? (double)sample_rate : 0.0, original_cols, nullptr,
                                            &entries_above_threshold, &avg_doc_sz, nullptr, &entries_in_A);
    feed_failed = false;
    after_matrices_built();
  }

  // src/trainer.cpp:425-654 (thresholding already done where the data came in): the hot path :490-571, then catchwords and topic vectors
  void train() {
    if (!is_data_loaded) throw std::runtime_error("train() before the data is loaded");
    log->print("Frob(B_fl_CSC): " + std::to_string(B_fl_CSC->frobenius()) + "\n");
    B_fl_CSC->initialize_for_eigensolver(num_topics);
    log->next_time_secs("eigen solver init");
    B_fl_CSC->compute_block_ks(num_topics, evalues);
    {
      std::ostringstream ostr;  // include/logUtils.h:101-122
      ostr << "Eigvals:  ";
      for (doc_id_t t = 0; t < num_topics; ++t) ostr << "(" << t << "): " << std::sqrt(evalues[t]) << "\t";
      ostr << std::endl;
      std::vector<FPTYPE> slabs(num_topics / 100 + 1, 0.0);
      for (doc_id_t t = 0; t < num_topics; ++t) slabs[t / 100] += evalues[t];
      for (doc_id_t slab = 0; slab < num_topics / 100; ++slab)
        ostr << "Sum of Top-" << (slab + 1) * 100 << " eig vals: " << std::accumulate(slabs.begin(), slabs.begin() + 1 + slab, (FPTYPE)0.0) << "\n";
      log->print(ostr.str());
    }
    log->next_time_secs("Spectra eigen solve");  // the reference uses this label for block-KS too (App. C #13)

    std::vector<doc_id_t> best_kmeans_seeds;
    FPTYPE* centers_lowd = new FPTYPE[(size_t)num_topics * num_topics];
    log->print("k-means init method: KMEANSPP\n");
    const FPTYPE best_residual = B_fl_CSC->kmeans_init_on_projected_space((int)num_topics, 1, best_kmeans_seeds, centers_lowd);
    log->print("Best k-means init residual: " + std::to_string(best_residual) + "\n");
    log->next_time_secs("K-means seeds initialization");

    B_fl_CSC->run_lloyds_on_projected_space(num_topics, centers_lowd, NULL, 10);
    // The reference allocates centers[vocab_size * num_topics] here (src/trainer.cpp:284) and hands it through both calls below, but
    // reads nothing of it afterwards (only closest_docs, :566-575): the lifted centres and Lloyd's result stay in device memory.
    FPTYPE* centers = nullptr;
    B_fl_CSC->left_multiply_by_U_Spectra(centers, centers_lowd, num_topics, num_topics);
    delete[] centers_lowd;
    log->next_time_secs("Converging LLoyds k-means on B_k");
    B_fl_CSC->cleanup_after_eigensolver();

    closest_docs = new std::vector<doc_id_t>[num_topics];
    B_fl_CSC->run_lloyds(num_topics, centers, closest_docs, 10);
    uint64_t closest_docs_sizes_sum = 0;
    for (doc_id_t t = 0; t < num_topics; ++t) closest_docs_sizes_sum += closest_docs[t].size();
    if (closest_docs_sizes_sum != B_fl_CSC->num_docs()) throw std::runtime_error("partition incomplete");  // :567-570
    log->next_time_secs("k-means on B");
    for (doc_id_t topic = 0; topic != num_topics; ++topic)  // :573-575
      for (auto d = closest_docs[topic].begin(); d < closest_docs[topic].end(); ++d) *d = original_cols[*d];
    {
      std::ofstream o(log_dir + "/HotPathClusters.tsv");  // topic \t doc, 1-based like the reference's sparse writers
      for (doc_id_t t = 0; t < num_topics; ++t)
        for (doc_id_t d : closest_docs[t]) o << (t + 1) << "\t" << (d + 1) << "\n";
      std::ofstream sv(log_dir + "/HotPathSingularValues.txt");
      sv << std::setprecision(9);
      for (doc_id_t t = 0; t < num_topics; ++t) sv << std::sqrt(evalues[t]) << "\n";
    }

    // ---- src/trainer.cpp:577-654: catchwords and the topic model, on the device ------------------
    uint64_t r;  // :579-583
    if (flag_sample_docs)
      r = (uint64_t)std::floor(ISLE_EPS2_C * ISLE_W0_C * (FPTYPE)num_docs * sample_rate / (FPTYPE)(2.0 * num_topics));
    else
      r = (uint64_t)std::floor(ISLE_EPS2_C * ISLE_W0_C * (FPTYPE)num_docs / (FPTYPE)(2.0 * num_topics));
    catchword_thresholds = new FPTYPE[(size_t)vocab_size * num_topics];
    catchwords = new std::vector<word_id_t>[num_topics];
    B_fl_CSC->find_catchwords(num_topics, r, catchword_thresholds, catchwords);
    log->next_time_secs("Collecting word freqs in clusters");
    log->next_time_secs("Finding catchwords for clusters");
    Model = new FPTYPE[(size_t)vocab_size * num_topics];
    // the documents' top-two topics stay on the device, where train_edge_topics() selects the pairs; the host loop beyond the counting table's limit needs them here
    B_fl_CSC->construct_topic_model(Model, num_topics, num_docs,
                                    flag_construct_edge_topics && flag_print_top_two_topics && num_topics > ISLE_EDGE_TABLE_MAX_TOPICS ? &top_topic_pairs : NULL);  // :648
    log->next_time_secs("Constructing topic vectors");
    is_training_complete = true;
  }

  void load_vocab() {  // create_vocab_list, src/utils.cpp:6-25 (once)
    if (!vocab_words.empty()) return;
    std::ifstream in(vocab_file);
    std::string word;
    const word_id_t lines = kept_words.empty() ? vocab_size : vocab_file_words;
    while (in.good() && !in.eof() && vocab_words.size() < lines) {
      in >> word;
      vocab_words.push_back(word);
    }
    vocab_words.resize(lines);
    if (!kept_words.empty()) {  // after prune_vocabulary(): word w of the model is line kept_words[w] of the file
      std::vector<std::string> kept(vocab_size);
      for (word_id_t w = 0; w < vocab_size; ++w) kept[w] = vocab_words[kept_words[w]];
      vocab_words.swap(kept);
    }
  }

  // The vocabulary pruned by document frequency, on the device (FPSparseMatrixHip::prune_vocabulary -> isle_hip_prune_vocab; the rule:
  // isle_amd/csrc/vocab_host.h): words in fewer than min_df or more than max_df (0: no upper bound) documents go, of the rest the keep_n
  // (0: no cap) most frequent stay.  After the data is loaded and before train(): A is compacted, B is thresholded again from it, vocab_size
  // becomes the kept words' number and load_vocab() maps the vocabulary file's lines through the kept words, so that every file that prints
  // words names the right ones.  VocabKept.tsv: new id, old id, df, the ids 1-based like the other writers.  Nothing in the CLI calls it.
  void prune_vocabulary(const uint64_t min_df, const uint64_t max_df = 0, const uint64_t keep_n = 0) {
    if (!is_data_loaded) throw std::runtime_error("prune_vocabulary() before the data is loaded");
    if (is_training_complete) throw std::runtime_error("prune_vocabulary() after train()");
    const word_id_t old_vocab = vocab_size;
    const uint64_t old_entries = entries_in_A;
    std::vector<uint32_t> kept, df;
    uint64_t entries = 0, emptied = 0;
    B_fl_CSC->prune_vocabulary(min_df, max_df, keep_n, kept, &df, &entries, &emptied);
    std::vector<uint32_t> lines(kept);  // the old id as the vocabulary file numbers it: a second prune goes through the first one's lines
    if (kept_words.empty()) vocab_file_words = old_vocab;
    else
      for (uint32_t& w : lines) w = kept_words[w];
    {
      FILE* f = std::fopen((log_dir + "/VocabKept.tsv").c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + log_dir + "/VocabKept.tsv");
      for (size_t w = 0; w < kept.size(); ++w) std::fprintf(f, "%llu\t%llu\t%u\n", (unsigned long long)w + 1, (unsigned long long)lines[w] + 1, df[kept[w]]);
      std::fclose(f);
    }
    kept_words.swap(lines);
    vocab_size = (word_id_t)kept_words.size();
    entries_in_A = entries;
    vocab_words.clear();
    B_fl_CSC->threshold_again(num_topics, flag_sample_docs ? (double)sample_rate : 0.0, original_cols, &entries_above_threshold, &avg_doc_sz);
    log->print("Vocabulary pruned: words kept " + std::to_string(vocab_size) + " dropped " + std::to_string(old_vocab - vocab_size) + ", entries kept " +
               std::to_string(entries) + " dropped " + std::to_string(old_entries - entries) + ", documents emptied " + std::to_string(emptied) + "\n");
    log->next_time_secs("Pruning the vocabulary");
  }

  // The documents pruned by length and as exact duplicates, on the device (FPSparseMatrixHip::prune_documents -> isle_hip_prune_docs; the
  // rule: isle_amd/csrc/docs_host.h): documents of fewer than min_words or more than max_words distinct words, of fewer than min_tokens
  // or more than max_tokens tokens go (a maximum of 0: no upper bound), and with drop_duplicates every document whose column equals an
  // earlier one's bit for bit.  After the data is loaded and before train(): A is compacted, B is thresholded again from it and num_docs
  // becomes the kept documents' number.  DocsKept.tsv: new id, old id (the document's number when the data was loaded), words, tokens,
  // the ids 1-based like the other writers.  FROM THEN ON EVERY PER-DOCUMENT REPORT PRINTS THE NEW NUMBERS: DocsKept.tsv is the way
  // back.  Nothing in the CLI calls it.
  void prune_documents(const uint64_t min_words, const uint64_t max_words = 0, const uint64_t min_tokens = 0, const uint64_t max_tokens = 0,
                       const bool drop_duplicates = false) {
    if (!is_data_loaded) throw std::runtime_error("prune_documents() before the data is loaded");
    if (is_training_complete) throw std::runtime_error("prune_documents() after train()");
    const doc_id_t old_docs = num_docs;
    const uint64_t old_entries = entries_in_A;
    std::vector<uint32_t> kept, words;
    std::vector<uint64_t> tokens;
    uint64_t entries = 0, dropped[3] = {0, 0, 0};
    B_fl_CSC->prune_documents(min_words, max_words, min_tokens, max_tokens, drop_duplicates, kept, nullptr, &entries, dropped);
    B_fl_CSC->doc_lengths(words, tokens);  // of the kept documents, in the new numbering
    if (!kept_docs.empty())                // a second prune goes through the first one's numbers
      for (uint32_t& d : kept) d = kept_docs[d];
    {
      FILE* f = std::fopen((log_dir + "/DocsKept.tsv").c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + log_dir + "/DocsKept.tsv");
      for (size_t d = 0; d < kept.size(); ++d)
        std::fprintf(f, "%llu\t%llu\t%u\t%llu\n", (unsigned long long)d + 1, (unsigned long long)kept[d] + 1, words[d], (unsigned long long)tokens[d]);
      std::fclose(f);
    }
    kept_docs.swap(kept);
    num_docs = (doc_id_t)kept_docs.size();
    entries_in_A = entries;
    B_fl_CSC->threshold_again(num_topics, flag_sample_docs ? (double)sample_rate : 0.0, original_cols, &entries_above_threshold, &avg_doc_sz);
    log->print("Documents pruned: kept " + std::to_string(num_docs) + " of " + std::to_string(old_docs) + ", too short " + std::to_string(dropped[0]) +
               ", too long " + std::to_string(dropped[1]) + ", duplicates " + std::to_string(dropped[2]) + ", entries kept " + std::to_string(entries) +
               " dropped " + std::to_string(old_entries - entries) + "\n");
    log->next_time_secs("Pruning the documents");
  }

  // The near duplicates pruned, on the device (FPSparseMatrixHip::prune_near_duplicates -> isle_hip_prune_near_docs; the rule:
  // isle_amd/csrc/neardup_host.h): every document whose word set has Jaccard similarity >= num/den with an earlier document that MinHash
  // banding (bands x rows_per_band) made its candidate goes.  After the data is loaded and before train(), like prune_documents: A is
  // compacted, B is thresholded again from it, num_docs becomes the kept documents' number and kept_docs stays up to date, so the
  // per-document reports print the new numbers.  DocsKept.tsv as prune_documents writes it.  NearDuplicates.tsv: one line per dropped
  // document, doc, parent, first_of, inter, uni: the ids 1-based and the numbers the documents had when the data was loaded, inter and uni
  // those of (doc, parent), taken before the prune.  Nothing in the CLI calls it.
  void prune_near_duplicates(const uint64_t num = 4, const uint64_t den = 5, const int bands = 16, const int rows_per_band = 4) {
    if (!is_data_loaded) throw std::runtime_error("prune_near_duplicates() before the data is loaded");
    if (is_training_complete) throw std::runtime_error("prune_near_duplicates() after train()");
    const doc_id_t old_docs = num_docs;
    const uint64_t old_entries = entries_in_A;
    std::vector<uint32_t> kept, parent, first_of, inter, uni, words;
    std::vector<uint64_t> tokens;
    uint64_t entries = 0;
    B_fl_CSC->prune_near_duplicates(num, den, bands, rows_per_band, kept, parent, first_of, &inter, &uni, &entries);
    B_fl_CSC->doc_lengths(words, tokens);  // of the kept documents, in the new numbering
    const auto loaded = [&](uint32_t d) { return (unsigned long long)(kept_docs.empty() ? d : kept_docs[d]) + 1; };  // a second prune goes through the first one's numbers
    {
      FILE* f = std::fopen((log_dir + "/NearDuplicates.tsv").c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + log_dir + "/NearDuplicates.tsv");
      for (size_t d = 0; d < first_of.size(); ++d)
        if (first_of[d] != d) std::fprintf(f, "%llu\t%llu\t%llu\t%u\t%u\n", loaded((uint32_t)d), loaded(parent[d]), loaded(first_of[d]), inter[d], uni[d]);
      std::fclose(f);
    }
    if (!kept_docs.empty())
      for (uint32_t& d : kept) d = kept_docs[d];
    {
      FILE* f = std::fopen((log_dir + "/DocsKept.tsv").c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + log_dir + "/DocsKept.tsv");
      for (size_t d = 0; d < kept.size(); ++d)
        std::fprintf(f, "%llu\t%llu\t%u\t%llu\n", (unsigned long long)d + 1, (unsigned long long)kept[d] + 1, words[d], (unsigned long long)tokens[d]);
      std::fclose(f);
    }
    kept_docs.swap(kept);
    num_docs = (doc_id_t)kept_docs.size();
    entries_in_A = entries;
    B_fl_CSC->threshold_again(num_topics, flag_sample_docs ? (double)sample_rate : 0.0, original_cols, &entries_above_threshold, &avg_doc_sz);
    log->print("Near duplicates pruned: kept " + std::to_string(num_docs) + " of " + std::to_string(old_docs) + " at " + std::to_string(num) + "/" + std::to_string(den) +
               ", " + std::to_string(bands) + " bands of " + std::to_string(rows_per_band) + ", entries kept " + std::to_string(entries) + " dropped " +
               std::to_string(old_entries - entries) + "\n");
    log->next_time_secs("Pruning the near duplicates");
  }

  // src/trainer.cpp:776-826
  void output_cluster_summary() {
    if (!is_training_complete) throw std::runtime_error("output_cluster_summary() before train()");
    load_vocab();
    const word_id_t ntop = std::min<word_id_t>(10, vocab_size);  // max(DEFAULT_COHERENCE_NUM_WORDS, 10), :781-783
    topwords.assign(num_topics, {});
    for (doc_id_t t = 0; t < num_topics; ++t) {  // DenseMatrix::find_n_top_words, src/denseMatrix.cpp:92-107 (ties: lower word id first)
      std::vector<std::pair<word_id_t, FPTYPE>>& tw = topwords[t];
      tw.reserve(vocab_size);
      for (word_id_t w = 0; w < vocab_size; ++w) tw.push_back(std::make_pair(w, Model[(size_t)t * vocab_size + w]));
      // heaviest first, lower word id first among equal weights (what a stable sort of the word-ordered list gives)
      std::partial_sort(tw.begin(), tw.begin() + ntop, tw.end(), [](const std::pair<word_id_t, FPTYPE>& l, const std::pair<word_id_t, FPTYPE>& r2) {
        return l.second > r2.second || (l.second == r2.second && l.first < r2.first);
      });
      if (tw[ntop - 1].second == (FPTYPE)0.0) std::cout << "\n ==== WARNING: top words in topic " << t << " have zero weight\n\n";
      tw.resize(ntop);
    }
    std::vector<double> coherences(num_topics, 0.0);
    double avg_coherence = 0.0;
    doc_id_t undefined = 0;
    if (flag_compute_avg_coherence) {
      B_fl_CSC->topic_coherence(num_topics, std::min<word_id_t>(ISLE_DEFAULT_COHERENCE_NUM_WORDS, ntop), topwords.data(), coherences);
      double sum = 0.0;
      for (doc_id_t t = 0; t < num_topics; ++t) {
        if (std::isfinite(coherences[t])) sum += coherences[t];
        else ++undefined;
      }
      avg_coherence = sum / (double)(num_topics - undefined);
      log->next_time_secs("Calculating coherence");
    }
    for (doc_id_t t = 0; t < num_topics; ++t) {
      std::ostringstream o;
      o << "\n---------- Topic: " << t << ", Cluster_size: " << closest_docs[t].size() << " -----------\n";
      o << "Catchwords:\n";  // include/logUtils.h:49-64
      for (word_id_t w : catchwords[t]) o << vocab_words[w] << ":" << w << "(" << catchword_thresholds[(size_t)t * vocab_size + w] << ") ";
      o << "\n";
      o << "\n#Top words: " << topwords[t].size() << "\n";  // src/denseMatrix.cpp:110-121
      for (auto& tw : topwords[t]) o << vocab_words[tw.first] << ":" << tw.first << "(" << tw.second << ") ";
      o << "\n\n";
      if (flag_compute_avg_coherence) o << "\nCoherence: " << std::to_string(coherences[t]) << "\n";  // :806
      log->diag << o.str();
    }
    log->diag << "\n---------------------------\n";
    if (flag_compute_avg_coherence) {
      if (undefined)
        log->print("\n Topics without a coherence (a top word occurs in no document): " + std::to_string(undefined) + "(" + std::to_string(num_topics) + ")\n");
      log->print("\n Avg coherence: " + std::to_string(avg_coherence) + "\n\n");
    } else {
      log->print("\n Avg coherence: " + std::to_string(0.0f) + "\n\n");
    }
    {  // LogUtils::print_cluster_details, include/logUtils.h:66-99
      std::vector<std::pair<int, doc_id_t>> cluster_sizes;
      for (doc_id_t t = 0; t < num_topics; ++t) cluster_sizes.push_back(std::make_pair((int)closest_docs[t].size(), t));
      std::stable_sort(cluster_sizes.begin(), cluster_sizes.end(),
                       [](const std::pair<int, doc_id_t>& l, const std::pair<int, doc_id_t>& r2) { return l.first < r2.first; });
      std::ostringstream o;
      int catchless = 0;
      for (doc_id_t i = 0; i < num_topics; ++i) {
        const doc_id_t t = cluster_sizes[i].second;
        o << std::setw(12) << std::left << "Cluster" << t << std::setw(12) << std::left << "  size:" << cluster_sizes[i].first << std::setw(15)
          << std::left << "  distsq_sum:" << 0 << std::setw(15) << std::left << "  raw_coh:" << 0 << std::setw(15) << std::left << "  flt_coh:";
        if (flag_compute_avg_coherence) o << coherences[t];  // topic t's own value (the reference prints coherences[i], i the sorted position)
        else o << 0;
        o << "  #catchwords: " << catchwords[t].size() << std::endl;
        if (catchwords[t].size() == 0) catchless++;
      }
      o << "\n#Topics with no catchwords: " << catchless << "(" << num_topics << ")" << std::endl;
      log->print(o.str());
    }
    log->next_time_secs("Output summary");
  }

  void output_top_words() {  // src/trainer.cpp:855-868
    std::ofstream out_top_words(log_dir + "/TopWordsPerTopic_catch.txt");
    for (doc_id_t t = 0; t < num_topics; ++t) {
      for (auto& tw : topwords[t]) out_top_words << vocab_words[tw.first] << "\t";
      out_top_words << std::endl;
    }
    log->next_time_secs("Writing top words to file");
  }
  void output_model(bool output_sparse = false) {  // src/trainer.cpp:831-838 (the CLI asks for the sparse form)
    (void)output_sparse;
    B_fl_CSC->write_model_text(ISLE_MODEL_CATCH, ISLE_TEXT_SPARSE, log_dir + "/M_hat_catch_sparse");
  }
  // src/trainer.cpp:656-662
  void write_model_to_file() {
    if (topwords.empty()) throw std::runtime_error("write_model_to_file() before output_cluster_summary()");
    output_top_words();
    output_model(true);
    log->next_time_secs("Output model");
    output_top_words();
    log->next_time_secs("Output topwords");
    if (flag_print_doctopic) output_doc_topic();  // :664-667, commented out in the reference
  }
  // src/trainer.cpp:874-991: DocCatchword.tsv and DocTopicCatchwordSums.tsv, formatted on the device (isle_hip_doc_report_text);
  // trainer_detail::doc_catchword_text / doc_topic_sums_text state the bytes
  void output_doc_topic() {
    if (!is_training_complete) throw std::runtime_error("output_doc_topic() before train()");
    uint64_t ncatch = 0;
    for (doc_id_t t = 0; t < num_topics; ++t) ncatch += catchwords[t].size();
    log->print("Total number of catchwords: " + std::to_string(ncatch) + "\n");
    B_fl_CSC->write_doc_report(log_dir + "/DocCatchword.tsv", ISLE_DOCREPORT_CATCHWORDS);
    B_fl_CSC->write_doc_report(log_dir + "/DocTopicCatchwordSums.tsv", ISLE_DOCREPORT_TOPIC_SUMS);
    log->next_time_secs("Writing document catchword weights");
  }
  // src/trainer.cpp:1008-1040: TopTwoTopicsPerDoc.txt from the resident top-two topics; trainer_detail::top_two_text states the bytes
  void print_top_two_topics() {
    if (!is_training_complete) throw std::runtime_error("print_top_two_topics() before train()");
    B_fl_CSC->write_doc_report(log_dir + "/TopTwoTopicsPerDoc.txt", ISLE_DOCREPORT_TOP_TWO);
  }
  const std::vector<word_id_t>* catchword_lists() const { return catchwords; }  // after train(): [num_topics], words ascending
  FPSparseMatrixHip* matrix() { return B_fl_CSC; }
  // src/trainer.cpp:673-685 -> construct_edge_topics_v2 :1116-1167
  void train_edge_topics() {
    if (!flag_construct_edge_topics) throw std::runtime_error("train_edge_topics() without construct_edge_topics");
    // without print_top_two_topics the reference collects no pairs (:648) and selects from none
    const bool on_host = !flag_print_top_two_topics || num_topics > ISLE_EDGE_TABLE_MAX_TOPICS;
    B_fl_CSC->construct_edge_topics(on_host ? &top_topic_pairs : nullptr, max_edge_topics, selected_pairs);
    EdgeModel.clear();
    edge_model_fetched = false;
    log->next_time_secs("Constructing edge topic model");
    print_edge_topic_composition();  // :1163-1166 (flag_print_edge_topic_composition, default true)
    print_edge_topic_top_words(10);
  }
  void print_edge_topic_composition() {  // :1169-1194
    std::ofstream out(log_dir + "/EdgeTopicComposition.txt", std::ios::binary);
    out << trainer_detail::edge_composition_text(selected_pairs);
  }
  // :1196-1245: 2 * num_top_words words of every edge topic, num_top_words of its two basic topics; min(., vocab_size) of each
  void print_edge_topic_top_words(const int num_top_words) {
    load_vocab();
    const word_id_t n_edge = std::min<word_id_t>(2 * (word_id_t)num_top_words, vocab_size), n_topic = std::min<word_id_t>((word_id_t)num_top_words, vocab_size);
    std::vector<uint32_t> e_ids, t_ids;
    std::vector<FPTYPE> e_w, t_w;
    B_fl_CSC->edge_top_words(selected_pairs, n_edge, e_ids, e_w);
    std::vector<std::vector<std::pair<word_id_t, FPTYPE>>> basic(num_topics);
    B_fl_CSC->model_top_words(ISLE_MODEL_CATCH, num_topics, n_topic, basic.data());
    for (doc_id_t t = 0; t < num_topics; ++t)
      for (auto& tw : basic[t]) {
        t_ids.push_back((uint32_t)tw.first);
        t_w.push_back(tw.second);
      }
    std::ofstream out(log_dir + "/EdgeTopicTopWords.txt", std::ios::binary);
    out << trainer_detail::edge_top_words_text(selected_pairs, vocab_words, e_ids.data(), e_w.data(), n_edge, t_ids.data(), t_w.data(), n_topic);
  }
  // src/trainer.cpp:687-693
  void write_edgemodel_to_file() {
    B_fl_CSC->write_edge_model_text(FPSparseMatrixHip::pair_ids(selected_pairs), (FPTYPE)ISLE_EDGE_TOPIC_PRIMARY_RATIO, log_dir + "/EdgeModel_sparse");
    log->next_time_secs("Output edge model");
  }
  // src/trainer.cpp:705-745, the cluster-average model (no catchwords) on the device; see the header comment for the deviations
  void output_avg_topic_coherence(FPTYPE& avg_nl_coherence, std::vector<FPTYPE>& nl_coherences) {
    if (!is_training_complete) throw std::runtime_error("output_avg_topic_coherence() before train()");
    load_vocab();
    AvgModel.assign((size_t)vocab_size * num_topics, 0.0f);
    B_fl_CSC->construct_avg_topic_model(AvgModel.data(), num_topics);
    const word_id_t ntop = std::min<word_id_t>(std::max<word_id_t>(ISLE_DEFAULT_COHERENCE_NUM_WORDS, 10), vocab_size);
    avg_topwords.assign(num_topics, {});
    B_fl_CSC->model_top_words(ISLE_MODEL_AVG, num_topics, ntop, avg_topwords.data());
    std::vector<double> coherences;
    B_fl_CSC->topic_coherence(num_topics, std::min<word_id_t>(ISLE_DEFAULT_COHERENCE_NUM_WORDS, ntop), avg_topwords.data(), coherences);
    double sum = 0.0;
    doc_id_t undefined = 0;
    for (doc_id_t t = 0; t < num_topics; ++t) {
      if (std::isfinite(coherences[t])) sum += coherences[t];
      else ++undefined;
    }
    const double avg = sum / (double)(num_topics - undefined);
    nl_coherences.assign(coherences.begin(), coherences.end());
    avg_nl_coherence = (FPTYPE)avg;
    if (undefined)
      log->print("\n Topics without a coherence (a top word occurs in no document): " + std::to_string(undefined) + "(" + std::to_string(num_topics) + ")\n");
    log->print("\nAvg coherence without catchwords: " + std::to_string(avg) + "\n");
    log->next_time_secs("computing coherence without catchwords");
    B_fl_CSC->write_model_text(ISLE_MODEL_AVG, ISLE_TEXT_DENSE, log_dir + "/M_hat_avg");
    log->next_time_secs("Writing Mhat to file");
    std::ofstream out_top_words_avg(log_dir + "/TopWordsPerTopic_avg.txt");
    for (doc_id_t t = 0; t < num_topics; ++t) {
      for (auto& tw : avg_topwords[t]) out_top_words_avg << vocab_words[tw.first] << "\t";
      out_top_words_avg << std::endl;
    }
    out_top_words_avg.close();
    log->next_time_secs("Writing top words to file");
  }
  // src/trainer.cpp:750-774 on the catch model, in double (the stated formula; see the header comment)
  void output_topic_diversity() {
    if (!is_training_complete) throw std::runtime_error("output_topic_diversity() before train()");
    std::vector<double> dist;
    double avg = 0.0;
    B_fl_CSC->topic_diversity(ISLE_MODEL_CATCH, num_topics, dist, avg);
    log->print("\n Average topic diversity: " + std::to_string((FPTYPE)avg) + "\n\n");
    log->next_time_secs("Calculating diversity");
  }
  // The reference accepts print_doctopic and never uses it; this is what it asks for.  The topic weights of every document of A
  // under the resident model (ISLEInfer's iterations on the device, FPSparseMatrixHip::infer_documents) into DocTopicWeights.tsv:
  // "<doc>\t<topic>\t<weight>\n", 1-based, documents and topics ascending, topics with weight > 1 / num_topics of the converged
  // documents, <weight> as weight_text prints it; the entries stay on the device and the file is formatted there
  // (FPSparseMatrixHip::write_infer_text -> isle_hip_infer_text; trainer_detail::write_doc_topic_lines states the bytes).  Deviation from running ISLEInfer on M_hat_catch_sparse: the model is the fp32
  // model, not the file's six truncated digits.
  void output_doc_topic_weights(const int which = ISLE_MODEL_CATCH, const int iters = ISLE_INFER_ITERS_DEFAULT, const FPTYPE Lf = ISLE_INFER_LF_DEFAULT) {
    if (!is_training_complete) throw std::runtime_error("output_doc_topic_weights() before train()");
    const doc_id_t docs = B_fl_CSC->count_docs();
    const uint64_t nconv = B_fl_CSC->infer_documents_resident(which, 0, docs, iters, Lf);
    log->print("Number of docs for which inference converged: " + std::to_string(nconv) + " (of " + std::to_string(docs) + ")\n");
    log->next_time_secs("Inferring document topic weights");
    B_fl_CSC->write_infer_text(log_dir + "/DocTopicWeights.tsv", ISLE_DOCTEXT_ENTRIES, 0, docs, 1);
    log->next_time_secs("Writing document topic weights to file");
  }
  // The k-means objective of the partition train() ended with, on the thresholded matrix B: sum over the documents of a cluster of
  // |b_d - c_t|^2 with the centres run_lloyds left on the device (what the reference's lloyds_iter returns as its residual,
  // src/sparseMatrix.cpp:1649-1663, and never writes anywhere).  ClusterObjective.tsv: "<topic>\t<size>\t<distsq_sum>\n", topics 1-based,
  // the sum as %.9g; the log gets the total.  Not part of what ISLETrain writes by default.
  void output_kmeans_objective() {
    if (!is_training_complete) throw std::runtime_error("output_kmeans_objective() before train()");
    std::vector<double> sums(num_topics);
    std::vector<uint64_t> sizes(num_topics);
    double total = 0.0;
    B_fl_CSC->kmeans_objective(ISLE_SPACE_WORD, num_topics, sums.data(), &total, sizes.data());
    FILE* f = std::fopen((log_dir + "/ClusterObjective.tsv").c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + log_dir + "/ClusterObjective.tsv");
    for (doc_id_t t = 0; t < num_topics; ++t) std::fprintf(f, "%llu\t%llu\t%.9g\n", (unsigned long long)(t + 1), (unsigned long long)sizes[t], sums[t]);
    std::fclose(f);
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.9g", total);
    log->print(std::string("k-means objective on B: ") + buf + "\n");
    log->next_time_secs("Computing the k-means objective");
  }
  // "Which documents show topic t best": the n heaviest documents of every topic by their catchword sums (ISLE_TOPDOCS_SUMS) or, after
  // output_doc_topic_weights(), by their inferred weights (ISLE_TOPDOCS_INFER), selected on the device (FPSparseMatrixHip::topic_top_docs ->
  // isle_hip_topic_top_docs).  TopDocsPerTopic.tsv: topics ascending, within a topic the selected documents in order (the heavier value
  // first, the smaller document among bit-equal values), one line "<doc + 1>\t<topic + 1>\t<value>\n" per document as doc_line_text prints
  // it: a host loop over at most num_topics x n lines.  The reference has no such file; not part of what ISLETrain writes by default.
  void output_topic_top_docs(const int n = 10, const int source = ISLE_TOPDOCS_SUMS) {
    if (!is_training_complete) throw std::runtime_error("output_topic_top_docs() before train()");
    std::vector<uint32_t> docs, counts;
    std::vector<FPTYPE> values;
    B_fl_CSC->topic_top_docs(source, num_topics, n, 0, docs, values, counts);
    FILE* f = std::fopen((log_dir + "/TopDocsPerTopic.tsv").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + log_dir + "/TopDocsPerTopic.tsv");
    char text[40];
    for (doc_id_t t = 0; t < num_topics; ++t)
      for (uint32_t i = 0; i < counts[t]; ++i)
        std::fwrite(text, 1, trainer_detail::doc_line_text((uint64_t)docs[(size_t)t * n + i] + 1, (uint64_t)t + 1, values[(size_t)t * n + i], text), f);
    std::fclose(f);
    log->next_time_secs("Writing the heaviest documents of every topic");
  }
  // "Which documents are like this one": for every document of query_docs (at most ISLE_SIMDOCS_MAX_QUERIES) its n most similar documents
  // by the resident catchword sums, scored (measure: ISLE_SIM_*) and selected on the device (FPSparseMatrixHip::similar_documents ->
  // isle_hip_similar_docs); a document is not its own neighbour.  Call it when the topic model exists (after train()).  SimilarDocs.tsv: for
  // each query in the order given and each neighbour in list order (the higher score first, the smaller document among bit-equal scores)
  // one line "<query doc + 1>\t<doc + 1>\t<score>\n" as isle_hip_doc_line_text prints it.  The reference has no such file; not part of
  // what ISLETrain writes by default.
  void output_similar_docs(const std::vector<doc_id_t>& query_docs, const int n = 10, const int measure = ISLE_SIM_COSINE) {
    if (!is_training_complete) throw std::runtime_error("output_similar_docs() before train()");
    std::vector<uint32_t> docs, counts;
    std::vector<FPTYPE> scores;
    const std::vector<uint64_t> rows(query_docs.begin(), query_docs.end());
    B_fl_CSC->similar_documents(ISLE_TOPDOCS_SUMS, measure, num_topics, n, 0, rows, docs, scores, counts);
    FILE* f = std::fopen((log_dir + "/SimilarDocs.tsv").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + log_dir + "/SimilarDocs.tsv");
    char text[40];
    for (size_t q = 0; q < rows.size(); ++q)
      for (uint32_t i = 0; i < counts[q]; ++i) {
        const int len = isle_hip_doc_line_text(rows[q] + 1, (uint64_t)docs[q * (size_t)n + i] + 1, scores[q * (size_t)n + i], text);
        if (len < 0) {
          std::fclose(f);
          throw std::runtime_error("output_similar_docs: a score outside the domain of the line text");
        }
        std::fwrite(text, 1, (size_t)len, f);
      }
    std::fclose(f);
    log->next_time_secs("Writing the most similar documents of the query documents");
  }
  // "How much of the corpus is each topic, and how does that differ between its parts": the resident catchword sums added up by group of
  // documents on the device (FPSparseMatrixHip::topic_prevalence -> isle_hip_topic_prevalence; the rule: isle_amd/csrc/prevalence_host.h).
  // groups: one label per document (ISLE_GROUP_NONE: no group), or empty with num_groups = 1: the whole corpus.  Call it when the topic
  // model exists (after train()).  TopicPrevalence.tsv: one line per cell with count > 0, group ascending, then topic ascending,
  // "<group>\t<topic + 1>\t<docs>\t<with_topic>\t<dominant>\t<sum>\t<mean>\n": the group is the caller's label, the topic 1-based as in every
  // file of the trainer, docs the documents of the group, with_topic those that store the topic, dominant those whose heaviest topic it
  // is, sum and mean = sum / docs as %.17g.  Formatted on the host: at most 2^24 cells.  The reference has no such file; not part of
  // what ISLETrain writes by default.
  void output_topic_prevalence(const std::vector<uint32_t>& groups, const uint32_t num_groups = 1, const bool normalise = false) {
    if (!is_training_complete) throw std::runtime_error("output_topic_prevalence() before train()");
    const FPSparseMatrixHip::TopicPrevalence p = B_fl_CSC->topic_prevalence(ISLE_TOPDOCS_SUMS, num_topics, groups, num_groups, normalise);
    FILE* f = std::fopen((log_dir + "/TopicPrevalence.tsv").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + log_dir + "/TopicPrevalence.tsv");
    for (uint32_t g = 0; g < num_groups; ++g)
      for (doc_id_t t = 0; t < num_topics; ++t) {
        const size_t at = (size_t)g * num_topics + t;
        if (!p.count[at]) continue;
        std::fprintf(f, "%u\t%llu\t%llu\t%llu\t%llu\t%.17g\t%.17g\n", g, (unsigned long long)(t + 1), (unsigned long long)p.docs[g],
                     (unsigned long long)p.count[at], (unsigned long long)p.dominant[at], p.sum[at], p.sum[at] / (double)p.docs[g]);
      }
    std::fclose(f);
    log->next_time_secs("Writing the topic prevalence by document group");
  }
  // "How well does the model predict these words": every document's held-out score on the device under this run's catch model, with the
  // weights output_doc_topic_weights() left resident (call it first), normalised per document (FPSparseMatrixHip::score_documents ->
  // isle_hip_score_docs; the rule: isle_amd/csrc/score_host.h).  held: the CSC of the words to score, one column per document of the count
  // matrix (for document completion: the part of every document the weights were not fitted to); nullptr: the resident count matrix
  // itself, which is then an in-sample figure under the same two headings.  floor > 0: a word the model gives less than floor is scored at
  // floor; with 0 such an entry is left out and counted.  DocScores.tsv: trainer_detail::doc_scores_text states its bytes.  The log gets
  // the log-likelihood per token and the perplexity, totals summed ascending on the host.  The reference has no such output; not part of
  // what ISLETrain writes by default.
  void output_doc_scores(const FPSparseMatrixHip::HeldEntries* held = nullptr, const double floor = 0.0) {
    if (!is_training_complete) throw std::runtime_error("output_doc_scores() before train()");
    const doc_id_t docs = B_fl_CSC->count_docs();
    const FPSparseMatrixHip::DocScores s = B_fl_CSC->score_documents(ISLE_MODEL_CATCH, 0, docs, ISLE_SCORE_LOG, true, floor, held);
    const std::string text = trainer_detail::doc_scores_text(1, s.tokens, s.score, s.unscored_entries);
    FILE* f = std::fopen((log_dir + "/DocScores.tsv").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + log_dir + "/DocScores.tsv");
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    char num[40];
    std::snprintf(num, sizeof num, "%.17g", s.total_score / s.total_tokens);
    log->print(std::string("Held-out log-likelihood per token: ") + num + "\n");
    std::snprintf(num, sizeof num, "%.17g", s.perplexity);
    log->print(std::string("Perplexity: ") + num + "\n");
    log->next_time_secs("Scoring held-out words per document");
  }
  // "Is this model the same as that one": the model file model_file (format ISLE_TEXT_SPARSE / ISLE_TEXT_DENSE, vocab_size x num_topics, as
  // write_model_to_file writes it) is read on the device into the resident loaded model (FPSparseMatrixHip::load_model_file) and this
  // run's catch model (side a) is compared with it (side b): the L1 distances of all topic pairs in double and the greedy matching by
  // them, on the device (FPSparseMatrixHip::compare_models -> isle_hip_compare_models; the rule: isle_amd/csrc/match_host.h).
  // TopicMatch.tsv: trainer_detail::topic_match_text states its bytes.  The log gets the mean distance of the matched topics.  The
  // reference has no such output; not part of what ISLETrain writes by default.
  void output_model_comparison(const std::string& model_file, const int format = ISLE_TEXT_SPARSE) {
    if (!is_training_complete) throw std::runtime_error("output_model_comparison() before train()");
    B_fl_CSC->load_model_file(model_file, vocab_size, num_topics, format);
    const FPSparseMatrixHip::TopicMatch m = B_fl_CSC->compare_models(ISLE_MODEL_CATCH, ISLE_MODEL_LOADED);
    const std::string text = trainer_detail::topic_match_text(m.match_a, m.match_dist);
    FILE* f = std::fopen((log_dir + "/TopicMatch.tsv").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + log_dir + "/TopicMatch.tsv");
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    char mean[40];
    std::snprintf(mean, sizeof mean, "%.17g", m.mean_dist);
    log->print(std::string("Avg L1 distance of matched topics: ") + mean + " (" + std::to_string(m.n_matched) + " of " + std::to_string(num_topics) + " matched)\n");
    log->next_time_secs("Comparing the model with a model file");
  }
  void finish_log() { log->total("TVSD"); }  // the "Total time for TVSD" line the reference's train() ends with (:652)

  // src/trainer.cpp:993-996: vocab_size x num_topics floats, column-major (element (word, topic) at word + topic * vocab_size)
  void get_basic_model(FPTYPE* const basicModel) { std::memcpy(basicModel, Model, (size_t)vocab_size * num_topics * sizeof(FPTYPE)); }
  int get_num_edge_topics() { return (int)selected_pairs.size(); }                                                        // :998-1001
  void get_edge_model(FPTYPE* const edgeModel) {  // :1003-1007; the vocab_size x #edge matrix exists on the host from the first call on
    if (!edge_model_fetched) B_fl_CSC->edge_model(selected_pairs, EdgeModel);
    edge_model_fetched = true;
    std::memcpy(edgeModel, EdgeModel.data(), EdgeModel.size() * sizeof(FPTYPE));
  }
  const std::vector<FPTYPE>& eigenvalues() const { return evalues; }
  const std::vector<std::vector<std::pair<word_id_t, FPTYPE>>>& top_words() const { return topwords; }  // after output_cluster_summary()
  const std::vector<std::vector<std::pair<word_id_t, FPTYPE>>>& avg_top_words() const { return avg_topwords; }  // after output_avg_topic_coherence()
  const std::vector<FPTYPE>& avg_model() const { return AvgModel; }  // after output_avg_topic_coherence()
  const std::string& log_directory() const { return log_dir; }
  const std::vector<doc_id_t>* partition() const { return closest_docs; }
};

}  // namespace ISLE
