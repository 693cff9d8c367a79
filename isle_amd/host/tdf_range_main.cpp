// isle_amd/host/tdf_range_main.cpp — tdf_pump::file_range against a sink in host memory: no library, no GPU
// (tests/test_tdf_pump_range_cpu.py builds it with the address and undefined-behaviour sanitizers).
//   tdf_range_main <file> <piece_bytes> [<b> <e>]
// Without a range, every 0 <= b, e <= size + 1 in turn.  Each range goes through twice: with read() as it is, and with a reader that
// returns 1 .. 7 bytes at a time and fails with EINTR before every third call.  One line per range: "<b> <e> <bytes handed over, in hex>"
// ("-" for none).  Exit status 0 iff both readers gave the same bytes for every range and the sink never saw a second buffer asked for
// while one was out, a commit without one, or a commit above its capacity.  What the bytes should be is the test's to say.
#include <sys/stat.h>

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
bool run(const char* path, uint64_t piece, uint64_t b, uint64_t e, std::vector<char>* text) {
  HostSink sink(piece);
  uint64_t bytes = 0;
  const int rc = tdf_pump::file_range(path, b, e, [&](char** p, uint64_t* n) { return sink.acquire(p, n); }, [&](uint64_t n) { return sink.commit(n); },
                                      &bytes, Read());
  *text = sink.text;
  return rc == 0 && sink.violations == 0 && !sink.out && bytes == sink.text.size();
}

bool range(const char* path, uint64_t piece, uint64_t b, uint64_t e) {
  std::vector<char> plain, ragged;
  const bool ok = run<tdf_pump::PosixRead>(path, piece, b, e, &plain) && run<RaggedRead>(path, piece, b, e, &ragged) && plain == ragged;
  std::printf("%llu %llu ", (unsigned long long)b, (unsigned long long)e);
  if (plain.empty()) std::printf("-");
  for (char ch : plain) std::printf("%02x", (unsigned)(unsigned char)ch);
  std::printf("%s\n", ok ? "" : " DIFFERENT");
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 && argc != 5) {
    std::cerr << "usage: tdf_range_main <file> <piece_bytes> [<b> <e>]\n";
    return 2;
  }
  const uint64_t piece = strtoull(argv[2], nullptr, 10);
  if (piece == 0) {
    std::cerr << "tdf_range_main: <piece_bytes> must be positive\n";
    return 2;
  }
  try {
    bool ok = true;
    if (argc == 5) {
      ok = range(argv[1], piece, strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10));
    } else {
      struct stat st;
      if (::stat(argv[1], &st) != 0) throw std::runtime_error(std::string("cannot open ") + argv[1]);
      const uint64_t size = (uint64_t)st.st_size;
      for (uint64_t b = 0; b <= size + 1; ++b)
        for (uint64_t e = 0; e <= size + 1; ++e) ok = range(argv[1], piece, b, e) && ok;
    }
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "tdf_range_main failed: " << e.what() << std::endl;
    return 1;
  }
}
