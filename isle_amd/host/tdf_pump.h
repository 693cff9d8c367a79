// isle_amd/host/tdf_pump.h — a file into a sink that lends out buffers: the file loop of the tdf text stream, written once.
//
//   acquire(&buf, &cap)   the sink lends a buffer of cap > 0 bytes
//   commit(n)             the first n bytes of it are the next piece of the file (0: nothing, the buffer goes back)
//
// Both return 0, or a code that stops the pump and is returned as it is.  A buffer is filled to the brim before it is committed unless the
// file ends first: read() may return fewer bytes than asked for at any time (pipes, network file systems, signals) and that is no end of file;
// only a return of 0 is.  EINTR is retried.  The pump knows nothing of the library: FPSparseMatrixHip::from_tdf_file puts isle_hip_tdf_acquire
// / isle_hip_tdf_commit behind it, tdf_pump_main a sink in host memory.
//
// file_range(path, b, e, ...) hands the sink the lines of one byte range and nothing else: the part of a file that one rank of several
// counts (isle_hip_tdf_begin_counts).  A line is a maximal run of bytes that ends in '\n' or at the end of the file; the range [b, e) owns
// the lines whose first byte s satisfies b <= s < e.  So with b > 0 and text[b - 1] != '\n' the bytes through the first '\n' at or after b
// belong to the range before (none there: the range owns nothing), and the last owned line ends with the first '\n' at a position >= e - 1,
// or with the file.  b >= e owns nothing.  The ranges [size * r / N, size * (r + 1) / N), r = 0 .. N - 1, own every line once: their outputs
// side by side are the file.  Skipping and stopping are memchr on the host; the sink sees whole lines only.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

namespace tdf_pump {

// read() as the pump calls it; tests put a reader that returns short counts and EINTR in its place
struct PosixRead {
  long operator()(int fd, char* buf, size_t n) const { return (long)::read(fd, buf, n); }
};

// -> 0, or the sink's code.  Throws std::runtime_error where the file cannot be opened or read.  *bytes (nullable): bytes committed.
template <class Acquire, class Commit, class Read = PosixRead>
int file(const std::string& path, Acquire acquire, Commit commit, uint64_t* bytes = nullptr, Read rd = Read()) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) throw std::runtime_error("cannot open tdf file " + path + ": " + std::strerror(errno));
  uint64_t total = 0;
  int rc = 0;
  for (bool eof = false; !eof && rc == 0;) {
    char* buf = nullptr;
    uint64_t cap = 0;
    rc = acquire(&buf, &cap);
    if (rc) break;
    if (!buf || cap == 0) {
      ::close(fd);
      throw std::runtime_error("tdf_pump: the sink lent no buffer");
    }
    uint64_t got = 0;
    while (got < cap) {
      const long r = rd(fd, buf + got, (size_t)(cap - got));
      if (r < 0) {
        if (errno == EINTR) continue;
        const std::string why = std::strerror(errno);
        (void)commit(0);
        ::close(fd);
        throw std::runtime_error("read error on " + path + ": " + why);
      }
      if (r == 0) {
        eof = true;
        break;
      }
      got += (uint64_t)r;
    }
    rc = commit(got);
    if (rc == 0) total += got;
  }
  ::close(fd);
  if (bytes) *bytes = total;
  return rc;
}

namespace detail {
// read() until it returns something: > 0 bytes, 0 at the end of the file; throws on an error other than EINTR (the descriptor stays the caller's)
template <class Read>
uint64_t read_some(Read& rd, int fd, char* buf, uint64_t n, const std::string& path) {
  for (;;) {
    const long r = rd(fd, buf, (size_t)n);
    if (r >= 0) return (uint64_t)r;
    if (errno == EINTR) continue;
    throw std::runtime_error("read error on " + path + ": " + std::strerror(errno));
  }
}
}  // namespace detail

// The lines of `path` that the byte range [b, e) owns (the rule is at the top of this file), through the same sink.  -> 0, or the sink's
// code.  *bytes (nullable): bytes committed.  The file must be seekable.
template <class Acquire, class Commit, class Read = PosixRead>
int file_range(const std::string& path, uint64_t b, uint64_t e, Acquire acquire, Commit commit, uint64_t* bytes = nullptr, Read rd = Read()) {
  if (bytes) *bytes = 0;
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) throw std::runtime_error("cannot open tdf file " + path + ": " + std::strerror(errno));
  if (b >= e) {
    ::close(fd);
    return 0;
  }
  uint64_t total = 0;
  int rc = 0;
  char* buf = nullptr;  // the buffer on loan, if any
  try {
    // ---- skip: from b - 1 through the first '\n'.  Where text[b - 1] is that '\n', the line that begins at b is owned.
    char skip[4096];
    uint64_t left = 0;           // bytes of skip[] behind the '\n': the first owned bytes
    const char* left_at = skip;
    uint64_t at = b;             // position in the file of the next owned byte
    if (b > 0) {
      if (::lseek(fd, (off_t)(b - 1), SEEK_SET) < 0) throw std::runtime_error("cannot seek in " + path + ": " + std::strerror(errno));
      uint64_t pos = b - 1;
      for (bool found = false; !found;) {
        const uint64_t r = detail::read_some(rd, fd, skip, sizeof skip, path);
        if (r == 0) {  // the file ends inside the line that began before b
          ::close(fd);
          return 0;
        }
        if (const void* q = std::memchr(skip, '\n', (size_t)r)) {
          const uint64_t i = (uint64_t)(static_cast<const char*>(q) - skip);
          at = pos + i + 1;
          left_at = skip + i + 1;
          left = r - i - 1;
          found = true;
        }
        pos += r;
      }
      if (at >= e) {  // the first line that begins at or after b begins at or after e
        ::close(fd);
        return 0;
      }
    }
    // ---- deliver: what is left of skip[], then reads straight into the sink's buffers, through the first '\n' at a position >= e - 1
    uint64_t cap = 0, got = 0;
    for (bool done = false; !done && rc == 0;) {
      if (!buf) {
        rc = acquire(&buf, &cap);
        if (rc) {
          buf = nullptr;
          break;
        }
        if (!buf || cap == 0) {
          buf = nullptr;
          throw std::runtime_error("tdf_pump: the sink lent no buffer");
        }
        got = 0;
      }
      uint64_t r;
      if (left) {
        r = left < cap - got ? left : cap - got;
        std::memcpy(buf + got, left_at, (size_t)r);
        left_at += r;
        left -= r;
      } else {
        r = detail::read_some(rd, fd, buf + got, cap - got, path);
        if (r == 0) done = true;  // the end of the file ends the last line
      }
      if (r) {
        const uint64_t from = e - 1 > at ? e - 1 - at : 0;  // of these r bytes, the first that may be the closing '\n'
        if (from < r)
          if (const void* q = std::memchr(buf + got + from, '\n', (size_t)(r - from))) {
            r = (uint64_t)(static_cast<const char*>(q) - (buf + got)) + 1;
            done = true;
          }
        got += r;
        at += r;
      }
      if (got == cap || done) {
        buf = nullptr;  // the commit takes it back, whatever it returns
        rc = commit(got);
        if (rc == 0) total += got;
      }
    }
  } catch (...) {
    if (buf) (void)commit(0);
    ::close(fd);
    throw;
  }
  ::close(fd);
  if (bytes) *bytes = total;
  return rc;
}

}  // namespace tdf_pump
