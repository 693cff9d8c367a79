// isle_amd/host/tdf_pump_main.cpp — the file loop of tdf_pump.h against a sink in host memory: no library, no GPU
// (tests/test_tdf_pump_cpu.py builds it with the address and undefined-behaviour sanitizers).
//   tdf_pump_main <file> <piece_bytes>
// The sink lends two buffers of <piece_bytes> in turn and appends what is committed.  The file goes through twice: with read() as it is, and
// with a reader that returns 1 .. 7 bytes at a time and fails with EINTR before every third call.  Exit status 0 iff both results equal the
// file read whole and the sink never saw a second buffer asked for while one was out, a commit without one, or a commit above its capacity.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "tdf_pump.h"

namespace {

struct HostSink {
  std::vector<char> buf[2];
  std::vector<char> text;
  uint64_t cap;
  int turn = 0;
  bool out = false;
  int violations = 0;
  uint64_t commits = 0;
  explicit HostSink(uint64_t piece) : cap(piece) {
    buf[0].resize(piece);
    buf[1].resize(piece);
  }
  int acquire(char** p, uint64_t* n) {
    if (out) ++violations;
    out = true;
    *p = buf[turn].data();
    *n = cap;
    return 0;
  }
  int commit(uint64_t n) {
    if (!out || n > cap) {
      ++violations;
      return 1;
    }
    out = false;
    text.insert(text.end(), buf[turn].begin(), buf[turn].begin() + (long)n);
    if (n) turn ^= 1;
    ++commits;
    return 0;
  }
};

struct RaggedRead {
  uint64_t calls = 0;
  long operator()(int fd, char* buf, size_t n) {
    if (++calls % 3 == 0) {
      errno = EINTR;
      return -1;
    }
    const size_t want = 1 + (size_t)(calls % 7);
    return (long)::read(fd, buf, n < want ? n : want);
  }
};

template <class Read>
bool run(const char* path, uint64_t piece, const std::vector<char>& whole, const char* how) {
  HostSink sink(piece);
  uint64_t bytes = 0;
  const int rc = tdf_pump::file(path, [&](char** p, uint64_t* n) { return sink.acquire(p, n); }, [&](uint64_t n) { return sink.commit(n); }, &bytes, Read());
  const bool ok = rc == 0 && sink.violations == 0 && !sink.out && bytes == whole.size() && sink.text == whole;
  std::printf("%s: %llu bytes in %llu commits, rc %d, %d violations: %s\n", how, (unsigned long long)bytes, (unsigned long long)sink.commits, rc, sink.violations,
              ok ? "equal" : "DIFFERENT");
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::cerr << "usage: tdf_pump_main <file> <piece_bytes>\n";
    return 2;
  }
  const uint64_t piece = strtoull(argv[2], nullptr, 10);
  if (piece == 0) {
    std::cerr << "tdf_pump_main: <piece_bytes> must be positive\n";
    return 2;
  }
  try {
    std::vector<char> whole;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + argv[1]);
    char tmp[65536];
    for (size_t r; (r = std::fread(tmp, 1, sizeof tmp, f)) > 0;) whole.insert(whole.end(), tmp, tmp + r);
    std::fclose(f);
    const bool a = run<tdf_pump::PosixRead>(argv[1], piece, whole, "read");
    const bool b = run<RaggedRead>(argv[1], piece, whole, "short reads and EINTR");
    return a && b ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "tdf_pump_main failed: " << e.what() << std::endl;
    return 1;
  }
}
