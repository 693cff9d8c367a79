// isle_amd/host/tdf_file_main.cpp — FPSparseMatrixHip::from_tdf_file (the file streamed through tdf_pump.h and isle_hip_tdf_*) held to
// FPSparseMatrixHip::from_tdf of the same file read whole.  Test driver (tests/test_gpu_tdf_file_host_cpp.py).
//   tdf_file_main <file> <V> <D> <max_entries> <num_topics> <piece_bytes>
// Builds the thresholded matrix both ways, each on an object of its own, and compares what the two calls hand back bit for bit: the count
// matrix A (FPSparseMatrixHip::get_count_matrix), entries_in_A, entries_above_threshold, avg_doc_sz, original_cols, the shape of B.  Where both
// throw, compares what they say behind their "<call>: ".  Exit status 0 only if the two agree.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>

#include "fpsparse_hip.h"

using namespace ISLE;

namespace {
struct Built {
  std::unique_ptr<FPSparseMatrixHip> B;
  std::string said;  // the exception's message behind "<call>: ", if it threw
  bool threw = false;
  std::vector<doc_id_t> original_cols;
  uint64_t in_A = 0, above = 0;
  float avg = 0.f;
  std::vector<FPTYPE> counts;
  std::vector<uint32_t> rows;
  std::vector<int64_t> offs;
  template <class Make>
  void run(Make make) {
    try {
      B.reset(make(*this));
      float avg2 = 0.f;
      B->get_count_matrix(counts, rows, offs, &avg2);
      if (std::memcmp(&avg, &avg2, sizeof(float)) != 0) throw std::runtime_error("self: avg_doc_sz of the call and of the context differ");
    } catch (const std::exception& e) {
      threw = true;
      const std::string m = e.what();
      const size_t a = m.find(": "), b = a == std::string::npos ? a : m.find(": ", a + 2);
      said = b == std::string::npos ? m : m.substr(b + 2);  // "<what>: <call>: <message>"
    }
  }
};

std::vector<char> read_whole(const std::string& path) {
  std::vector<char> text;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open tdf file " + path);
  char tmp[65536];
  for (size_t r; (r = std::fread(tmp, 1, sizeof tmp, f)) > 0;) text.insert(text.end(), tmp, tmp + r);
  std::fclose(f);
  return text;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 7) {
    std::cerr << "usage: tdf_file_main <file> <V> <D> <max_entries> <num_topics> <piece_bytes>\n";
    return 2;
  }
  const std::string path = argv[1];
  const uint64_t V = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10), max_entries = strtoull(argv[4], nullptr, 10),
                 k = strtoull(argv[5], nullptr, 10), piece = strtoull(argv[6], nullptr, 10);
  try {
    const std::vector<char> text = read_whole(path);
    Built w, s;
    w.run([&](Built& o) {
      return FPSparseMatrixHip::from_tdf(V, D, text.data(), text.size(), (offset_t)max_entries, k, 0.0, o.original_cols, &o.in_A, &o.above, &o.avg);
    });
    s.run([&](Built& o) { return FPSparseMatrixHip::from_tdf_file(V, D, path, (offset_t)max_entries, k, 0.0, o.original_cols, &o.in_A, &o.above, &o.avg, 0, piece); });
    if (w.threw != s.threw || w.said != s.said) {
      std::cerr << "tdf_file_main: from_tdf_file " << (s.threw ? "says \"" + s.said + "\"" : std::string("accepts the file")) << ", from_tdf "
                << (w.threw ? "says \"" + w.said + "\"" : std::string("accepts it")) << std::endl;
      return 1;
    }
    if (s.threw) {
      std::printf("both refuse: %s\n", s.said.c_str());
      return 0;
    }
    const bool same = s.in_A == w.in_A && s.above == w.above && std::memcmp(&s.avg, &w.avg, sizeof(float)) == 0 && s.original_cols == w.original_cols &&
                      s.B->num_docs() == w.B->num_docs() && s.B->get_nnzs() == w.B->get_nnzs() && s.B->count_docs() == w.B->count_docs() && s.offs == w.offs &&
                      s.rows == w.rows && s.counts.size() == w.counts.size() &&
                      (s.counts.empty() || std::memcmp(s.counts.data(), w.counts.data(), s.counts.size() * sizeof(FPTYPE)) == 0);
    if (!same) {
      std::cerr << "tdf_file_main: the two differ: entries_in_A " << s.in_A << " / " << w.in_A << ", above threshold " << s.above << " / " << w.above << ", avg_doc_sz "
                << s.avg << " / " << w.avg << ", documents of B " << s.B->num_docs() << " / " << w.B->num_docs() << ", nnz of B " << s.B->get_nnzs() << " / "
                << w.B->get_nnzs() << " (from_tdf_file / from_tdf)" << std::endl;
      return 1;
    }
    std::printf("identical: entries_in_A %llu, above threshold %llu, B %llu documents, %lld entries\n", (unsigned long long)s.in_A, (unsigned long long)s.above,
                (unsigned long long)s.B->num_docs(), (long long)s.B->get_nnzs());
  } catch (const std::exception& e) {
    std::cerr << "tdf_file_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
