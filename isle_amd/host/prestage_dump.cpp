// isle_amd/host/prestage_dump.cpp — CPU-only helper for tests: runs the ISLETrain pre-stages (tdf -> A -> B) and dumps B, or stops at A.
//   prestage_dump <tdf> <vocab_size> <num_docs> <max_entries> <num_topics> <sample_rate or 0> <out.bin>
// out.bin: u64 V, u64 D_B, u64 nnz, u64 entries_above_threshold, f32 vals[nnz], u64 rows[nnz], i64 offs[D_B+1], u64 original_cols[D_B], f32 zetas[V]
//   prestage_dump --A <tdf> <vocab_size> <num_docs> <max_entries> <out.bin>
// out.bin: u64 V, u64 D, u64 nnz, f32 counts[nnz], u64 rows[nnz], i64 offs[D+1]
// A rejected line ends either form with "tdf file: <kind> on line <1-based line>" on stderr and exit status 1.
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "prestage.h"

int main(int argc, char** argv) {
  const bool only_A = argc == 7 && std::strcmp(argv[1], "--A") == 0;
  if (!only_A && argc != 8) return 2;
  try {
    using namespace ISLE::prestage;
    if (only_A) ++argv;  // the five arguments after --A sit where the first five of the long form do
    const uint64_t V = std::strtoull(argv[2], nullptr, 10), D = std::strtoull(argv[3], nullptr, 10);
    std::vector<DocWordEntry> e;
    read_tdf(argv[1], std::strtoull(argv[4], nullptr, 10), e, V, D);
    Csc A;
    float avg;
    uint64_t nz;
    build_A(e, V, D, A, &avg, &nz);
    if (only_A) {
      FILE* o = std::fopen(argv[5], "wb");
      if (!o) throw std::runtime_error(std::string("cannot write ") + argv[5]);
      uint64_t hdr[3] = {A.V, A.D, (uint64_t)A.offs.back()};
      std::fwrite(hdr, 8, 3, o);
      std::fwrite(A.vals.data(), 4, A.vals.size(), o);
      std::fwrite(A.rows.data(), 8, A.rows.size(), o);
      std::fwrite(A.offs.data(), 8, A.offs.size(), o);
      std::fclose(o);
      return 0;
    }
    Thresholded T;
    threshold(A, avg, nz, std::atol(argv[5]), std::atof(argv[6]), 0, T);
    FILE* o = std::fopen(argv[7], "wb");
    uint64_t hdr[4] = {T.B.V, T.B.D, (uint64_t)T.B.offs.back(), T.entries_above_threshold};
    std::fwrite(hdr, 8, 4, o);
    std::fwrite(T.B.vals.data(), 4, T.B.vals.size(), o);
    std::fwrite(T.B.rows.data(), 8, T.B.rows.size(), o);
    std::fwrite(T.B.offs.data(), 8, T.B.offs.size(), o);
    std::fwrite(T.original_cols.data(), 8, T.original_cols.size(), o);
    std::fwrite(T.zetas.data(), 4, T.zetas.size(), o);
    std::fclose(o);
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << std::endl;
    return 1;
  }
  return 0;
}
