// isle_amd/host/tdf_pump.h — a file into a sink that lends out buffers: the file loop of the tdf text stream, written once.
//
//   acquire(&buf, &cap)   the sink lends a buffer of cap > 0 bytes
//   commit(n)             the first n bytes of it are the next piece of the file (0: nothing, the buffer goes back)
//
// Both return 0, or a code that stops the pump and is returned as it is.  A buffer is filled to the brim before it is committed unless the
// file ends first: read() may return fewer bytes than asked for at any time (pipes, network file systems, signals) and that is no end of file;
// only a return of 0 is.  EINTR is retried.  The pump knows nothing of the library: FPSparseMatrixHip::from_tdf_file puts isle_hip_tdf_acquire
// / isle_hip_tdf_commit behind it, tdf_pump_main a sink in host memory.
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

}  // namespace tdf_pump
