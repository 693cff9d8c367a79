// isle_amd/host/feed_main.cpp — the device feed (isle_hip_feed_begin / _entries / _finalize through FPSparseMatrixHip's C ABI) held to the
// host statement of its rule, trainer_detail::csc_from_fed (trainer_hip.h).  Test driver (tests/test_gpu_feed_host_cpp.py) and the timing
// of tools/feed_probe.py.
//   feed_main <tdf> <V> <D> <flush_entries> [--time]
// Reads "<doc> <word> <count>" lines (1-based ids; a count of 0 is allowed here, unlike in isle_hip_ingest_tdf: the feed skips it), shuffles
// the documents and the words within each with a fixed seed, and builds A twice from that order: csc_from_fed on the host (zero counts left
// out first, as ISLETrainer::feed_data does), and the device feed in batches of <flush_entries>.  The device A is fetched with isle_hip_get_A;
// exit status 1, naming the first differing element, if the two differ in any bit.  --time: one JSON line with both walls — host =
// csc_from_fed + isle_hip_upload_counts_u32 (the path finalize_data took before the device feed), device = feed_begin .. feed_finalize;
// each side on a context of its own that has done one tiny call of the same kind before its wall starts.
#include <random>

#include "trainer_hip.h"

using namespace ISLE;

namespace {
double seconds_since(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
struct Ctx {
  isle_ctx* c;
  Ctx() : c(isle_hip_create(0)) {
    if (!c) throw std::runtime_error("isle_hip_create failed: no MI355X device");
  }
  ~Ctx() { isle_hip_destroy(c); }
  void check(int rc, const char* what) const {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + isle_hip_last_error(c));
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 5 || argc > 6 || (argc == 6 && std::string(argv[5]) != "--time")) {
    std::cerr << "usage: feed_main <tdf> <V> <D> <flush_entries> [--time]\n";
    return 2;
  }
  const uint64_t V = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10), flush = strtoull(argv[4], nullptr, 10);
  const bool timed = argc == 6;
  if (V == 0 || D == 0 || flush == 0) {
    std::cerr << "feed_main: <V>, <D> and <flush_entries> must be positive\n";
    return 2;
  }
  try {
    // ---- the triples, in shuffled document order with each document's words shuffled
    std::vector<uint32_t> doc, word, cnt;
    {
      std::vector<uint32_t> fd, fw, fc;
      FILE* f = std::fopen(argv[1], "r");
      if (!f) throw std::runtime_error(std::string("cannot open ") + argv[1]);
      unsigned long long d, w, x;
      while (std::fscanf(f, "%llu %llu %llu", &d, &w, &x) == 3) {
        if (d < 1 || d > D || w < 1 || w > V || x > 0xffffffffull) {
          std::fclose(f);
          throw std::runtime_error("entry " + std::to_string(fd.size()) + " of the file is out of range");
        }
        fd.push_back((uint32_t)(d - 1));
        fw.push_back((uint32_t)(w - 1));
        fc.push_back((uint32_t)x);
      }
      std::fclose(f);
      const size_t n = fd.size();
      std::vector<uint64_t> start(D + 1, 0);
      for (size_t i = 0; i < n; ++i) start[fd[i] + 1]++;
      for (uint64_t j = 0; j < D; ++j) start[j + 1] += start[j];
      std::vector<size_t> by_doc(n);  // file positions grouped by document, file order within
      {
        std::vector<uint64_t> cur(start.begin(), start.end() - 1);
        for (size_t i = 0; i < n; ++i) by_doc[cur[fd[i]]++] = i;
      }
      std::mt19937_64 rng(5);
      std::vector<uint64_t> order(D);
      std::iota(order.begin(), order.end(), (uint64_t)0);
      std::shuffle(order.begin(), order.end(), rng);
      doc.reserve(n);
      word.reserve(n);
      cnt.reserve(n);
      for (uint64_t j : order) {
        std::shuffle(by_doc.begin() + start[j], by_doc.begin() + start[j + 1], rng);
        for (uint64_t at = start[j]; at < start[j + 1]; ++at) {
          doc.push_back(fd[by_doc[at]]);
          word.push_back(fw[by_doc[at]]);
          cnt.push_back(fc[by_doc[at]]);
        }
      }
    }
    const size_t n = doc.size();

    // ---- host: the rule, then the finished CSC to the device
    std::vector<float> h_counts;
    std::vector<uint32_t> h_rows;
    std::vector<offset_t> h_offs;
    double host_s = 0;
    {
      Ctx up;
      std::vector<uint32_t> kd, kw, kc;  // what feed_data keeps: no zero counts (it drops them as they come in: outside the wall)
      kd.reserve(n);
      kw.reserve(n);
      kc.reserve(n);
      for (size_t i = 0; i < n; ++i)
        if (cnt[i]) {
          kd.push_back(doc[i]);
          kw.push_back(word[i]);
          kc.push_back(cnt[i]);
        }
      if (timed) {  // a context's first upload is not part of the wall, as the first launches below are not
        const float one = 1.f;
        const uint32_t row0 = 0;
        const offset_t o2[2] = {0, 1};
        up.check(isle_hip_upload_counts_u32(up.c, 1, 1, 1, &one, &row0, o2, 0, 1), "upload_counts");
        up.check(isle_hip_synchronize(up.c), "synchronize");
      }
      const auto t0 = std::chrono::steady_clock::now();
      trainer_detail::csc_from_fed(D, kd, kw, kc, h_counts, h_rows, h_offs);
      up.check(isle_hip_upload_counts_u32(up.c, V, D, h_counts.size(), h_counts.data(), h_rows.data(), h_offs.data(), 0, D), "upload_counts");
      up.check(isle_hip_synchronize(up.c), "synchronize");
      host_s = seconds_since(t0);
    }

    // ---- device: the same order in batches
    Ctx dev;
    if (timed) {  // the first launches of a context load the code object: not part of the wall
      const uint32_t z = 0, one = 1;
      dev.check(isle_hip_feed_begin(dev.c, 1, 1, 0), "feed_begin");
      dev.check(isle_hip_feed_entries(dev.c, 1, &z, &z, &one), "feed_entries");
      dev.check(isle_hip_feed_finalize(dev.c, 0, 0, nullptr, nullptr), "feed_finalize");
    }
    uint64_t fed = 0, nnz = 0;
    const auto t0 = std::chrono::steady_clock::now();
    dev.check(isle_hip_feed_begin(dev.c, V, D, n), "feed_begin");
    for (size_t at = 0; at < n; at += flush) {
      const size_t m = std::min<size_t>(flush, n - at);
      dev.check(isle_hip_feed_entries(dev.c, m, doc.data() + at, word.data() + at, cnt.data() + at), "feed_entries");
    }
    dev.check(isle_hip_feed_finalize(dev.c, 0, 0, &fed, &nnz), "feed_finalize");
    dev.check(isle_hip_synchronize(dev.c), "synchronize");
    const double dev_s = seconds_since(t0);

    if (nnz != h_counts.size()) {
      std::cerr << "feed_main: nnz differs: device " << nnz << ", host " << h_counts.size() << std::endl;
      return 1;
    }
    std::vector<float> g_counts(nnz);
    std::vector<uint32_t> g_rows(nnz);
    std::vector<offset_t> g_offs(D + 1);
    dev.check(isle_hip_get_A(dev.c, g_counts.data(), g_rows.data(), g_offs.data()), "get_A");
    for (uint64_t j = 0; j <= D; ++j)
      if (g_offs[j] != h_offs[j]) {
        std::cerr << "feed_main: offsets[" << j << "] differs: device " << g_offs[j] << ", host " << h_offs[j] << std::endl;
        return 1;
      }
    for (uint64_t i = 0; i < nnz; ++i) {
      if (g_rows[i] != h_rows[i]) {
        std::cerr << "feed_main: rows[" << i << "] differs: device " << g_rows[i] << ", host " << h_rows[i] << std::endl;
        return 1;
      }
      if (std::memcmp(&g_counts[i], &h_counts[i], sizeof(float)) != 0) {
        std::cerr << "feed_main: counts[" << i << "] differs: device " << g_counts[i] << ", host " << h_counts[i] << std::endl;
        return 1;
      }
    }
    if (timed)
      std::printf("{\"entries\": %llu, \"entries_fed\": %llu, \"nnz\": %llu, \"flush_entries\": %llu, \"host_csc_from_fed_plus_upload_s\": %.4f, \"device_feed_s\": %.4f}\n",
                  (unsigned long long)n, (unsigned long long)fed, (unsigned long long)nnz, (unsigned long long)flush, host_s, dev_s);
    else
      std::printf("identical: %llu entries fed, %llu kept, nnz %llu\n", (unsigned long long)n, (unsigned long long)fed, (unsigned long long)nnz);
  } catch (const std::exception& e) {
    std::cerr << "feed_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
