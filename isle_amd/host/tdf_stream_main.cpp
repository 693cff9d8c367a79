// isle_amd/host/tdf_stream_main.cpp — the tdf text stream (isle_hip_tdf_begin / _acquire / _commit / _finalize under tdf_pump.h's file loop) held
// to isle_hip_ingest_tdf of the same file read whole.  Test driver (tests/test_gpu_tdf_stream.py) and the C++ walls of tools/tdf_stream_probe.py.
//   tdf_stream_main <file> <V> <D> <piece_bytes> [--time | --time-stream-first]
// Streams the file in pieces of <piece_bytes> (0: the library's own size), ingests it whole on a second context, fetches both count matrices
// with isle_hip_get_A and compares them bit for bit; where both refuse the text, compares what they say of it (the kind and the line: the
// messages behind their "<call>: ").  Exit status 0 only if the two agree.  --time: one JSON line with both walls, file open to synchronised
// device — whole = what ISLETrainer::load_data_from_file did before it streamed (the file read into a vector, then isle_hip_ingest_tdf), stream =
// tdf_begin .. tdf_finalize; each on a context that has ingested one tiny text the same way before its wall starts.  The whole-text leg runs first,
// with --time-stream-first the stream: a caller that wants neither order favoured alternates the two.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../../include/isle_hip.h"
#include "tdf_pump.h"

namespace {
double seconds_since(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

struct Side {
  isle_ctx* c;
  int rc = 0;
  std::string said;  // the message behind "<call>: " when rc != 0
  uint64_t read = 0, nnz = 0;
  double wall = 0;
  std::vector<float> counts;
  std::vector<uint32_t> rows;
  std::vector<int64_t> offs;
  Side() : c(isle_hip_create(0)) {
    if (!c) throw std::runtime_error("isle_hip_create failed: no MI355X device");
  }
  ~Side() { isle_hip_destroy(c); }
  void done(int code, uint64_t D) {
    rc = code;
    if (rc) {
      const std::string m = isle_hip_last_error(c);
      const size_t at = m.find(": ");
      said = at == std::string::npos ? m : m.substr(at + 2);
      return;
    }
    counts.resize(nnz);
    rows.resize(nnz);
    offs.resize(D + 1);
    if (isle_hip_get_A(c, counts.data(), rows.data(), offs.data()) != 0) throw std::runtime_error(std::string("get_A: ") + isle_hip_last_error(c));
  }
};

int stream(isle_ctx* c, const std::string& path, uint64_t V, uint64_t D, uint64_t piece, uint64_t* read, uint64_t* nnz) {
  int rc = isle_hip_tdf_begin(c, V, D, 0, piece);
  if (rc == 0) rc = tdf_pump::file(path, [c](char** buf, uint64_t* cap) { return isle_hip_tdf_acquire(c, buf, cap); }, [c](uint64_t n) { return isle_hip_tdf_commit(c, n); });
  if (rc == 0) rc = isle_hip_tdf_finalize(c, 0, read, nnz);
  if (rc == 0) rc = isle_hip_synchronize(c);
  return rc;
}

int whole(isle_ctx* c, const std::string& path, uint64_t V, uint64_t D, uint64_t* read, uint64_t* nnz) {
  std::vector<char> text;  // as ISLETrainer::load_data_from_file read it before it streamed
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open tdf file " + path);
  std::fseek(f, 0, SEEK_END);
  const long sz = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  text.resize((size_t)sz);
  if (sz && std::fread(text.data(), 1, (size_t)sz, f) != (size_t)sz) {
    std::fclose(f);
    throw std::runtime_error("short read on " + path);
  }
  std::fclose(f);
  int rc = isle_hip_ingest_tdf(c, text.data(), text.size(), V, D, 0, read, nnz);
  if (rc == 0) rc = isle_hip_synchronize(c);
  return rc;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 5 || argc > 6 || (argc == 6 && std::string(argv[5]) != "--time" && std::string(argv[5]) != "--time-stream-first")) {
    std::cerr << "usage: tdf_stream_main <file> <V> <D> <piece_bytes> [--time | --time-stream-first]\n";
    return 2;
  }
  const std::string path = argv[1];
  const uint64_t V = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10), piece = strtoull(argv[4], nullptr, 10);
  const bool timed = argc == 6, stream_first = timed && std::string(argv[5]) == "--time-stream-first";
  try {
    Side s, w;
    if (timed) {  // the first launches of a context load the code object, the first stream page-locks its buffers: not part of the walls
      static const char tiny[] = "1 1 1\n";
      uint64_t a = 0, b = 0;
      if (isle_hip_tdf_begin(s.c, 1, 1, 0, piece) || isle_hip_tdf_write(s.c, tiny, 6) || isle_hip_tdf_finalize(s.c, 0, &a, &b) ||
          isle_hip_ingest_tdf(w.c, tiny, 6, 1, 1, 0, &a, &b))
        throw std::runtime_error("the warm-up ingest failed");
    }
    int wrc = 0, src = 0;
    for (int leg = 0; leg < 2; ++leg) {
      const auto t0 = std::chrono::steady_clock::now();
      if ((leg == 0) == stream_first) {
        src = stream(s.c, path, V, D, piece, &s.read, &s.nnz);
        s.wall = seconds_since(t0);
      } else {
        wrc = whole(w.c, path, V, D, &w.read, &w.nnz);
        w.wall = seconds_since(t0);
      }
    }
    w.done(wrc, D);
    s.done(src, D);
    if ((s.rc != 0) != (w.rc != 0) || s.said != w.said) {
      std::cerr << "tdf_stream_main: the stream " << (s.rc ? "says \"" + s.said + "\"" : std::string("accepts the text")) << ", the whole-text ingest "
                << (w.rc ? "says \"" + w.said + "\"" : std::string("accepts it")) << std::endl;
      return 1;
    }
    if (s.rc) {
      std::printf("both refuse: %s\n", s.said.c_str());
      return 0;
    }
    if (s.read != w.read || s.nnz != w.nnz) {
      std::cerr << "tdf_stream_main: entries read " << s.read << " / " << w.read << ", nnz " << s.nnz << " / " << w.nnz << " (stream / whole)" << std::endl;
      return 1;
    }
    for (uint64_t j = 0; j <= D; ++j)
      if (s.offs[j] != w.offs[j]) {
        std::cerr << "tdf_stream_main: offsets[" << j << "] differs: stream " << s.offs[j] << ", whole " << w.offs[j] << std::endl;
        return 1;
      }
    for (uint64_t i = 0; i < s.nnz; ++i)
      if (s.rows[i] != w.rows[i] || std::memcmp(&s.counts[i], &w.counts[i], sizeof(float)) != 0) {
        std::cerr << "tdf_stream_main: entry " << i << " differs: stream (" << s.rows[i] << ", " << s.counts[i] << "), whole (" << w.rows[i] << ", " << w.counts[i] << ")"
                  << std::endl;
        return 1;
      }
    if (timed)
      std::printf("{\"entries_read\": %llu, \"nnz\": %llu, \"piece_bytes\": %llu, \"stream_first\": %s, \"whole_read_plus_ingest_s\": %.4f, \"stream_s\": %.4f}\n", (unsigned long long)s.read,
                  (unsigned long long)s.nnz, (unsigned long long)piece, stream_first ? "true" : "false", w.wall, s.wall);
    else
      std::printf("identical: %llu entries read, nnz %llu\n", (unsigned long long)s.read, (unsigned long long)s.nnz);
  } catch (const std::exception& e) {
    std::cerr << "tdf_stream_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
