// isle_amd/host/ks_host_main.cpp — the host side of the block Krylov-Schur solver (../csrc/ks_host.h) replayed from a script on stdin, one
// JSON object per command on stdout: no library, no GPU (tests/test_ks_host_cpu.py builds it with the address and undefined-behaviour
// sanitizers and sends every input, so there is no generator here to keep in step).  Matrices arrive column-major, as the solver holds them.
//   consts                                   the mailbox constants
//   args nev ncv blk maxit dim               effective block width and the two argument checks
//   passes <text | ->                        ks_ortho_passes of the switch's text (- : unset)
//   mail cap_r blk npass m                   floats per mailbox, floats copied back
//   slice dim world                          the row slice of every rank
//   stage n keep nconv                       the staging layout of a truncation
//   blk b | ncv n | nev k                    set the case for the commands below
//   tight r c <r*c>                          H = HMat(r, c) with these entries
//   start rank <2*blk*blk> <rank*blk>        H = ks_h_start
//   reserve                                  ks_h_reserve; the expand loop's hr / hcn start at H.r / H.c
//   fold npass rk <npass*m*blk> <rk*blk>     ks_fold_step at (hr, hcn), then hr / hcn advance and H.r / H.c take them
//   truncate nconv <n> <n*keep> <nconv*keep> the two extracts, then H = ks_h_truncate(eH, vH, top)
//   unconv tol divide                        ks_first_unconverged
//   counts tol nconv last_j n_restarts maxit ks_final_counts
#include <cstdio>
#include <iostream>
#include <string>

#include "../csrc/ks_host.h"

namespace {

std::vector<float> take(size_t n) {
  std::vector<float> v(n);
  for (float& x : v) std::cin >> x;
  return v;
}
void put(const char* name, const float* v, size_t n) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) std::printf(i ? ",%.9g" : "%.9g", v[i]);
  std::printf("]");
}
// the r x c in use column by column, and whether the rest of the allocation is zero
void put(const HMat& H) {
  std::vector<float> a;
  bool rest_zero = true;
  for (size_t j = 0; j < H.cap_c; ++j)
    for (size_t i = 0; i < H.ld; ++i) {
      if (i < H.r && j < H.c) a.push_back(H(i, j));
      else if (H(i, j) != 0.f) rest_zero = false;
    }
  std::printf("\"r\": %zu, \"c\": %zu, \"ld\": %zu, \"cap_c\": %zu, \"alloc\": %zu, \"rest_zero\": %s, ", H.r, H.c, H.ld, H.cap_c, H.a.size(), rest_zero ? "true" : "false");
  put("a", a.data(), a.size());
}

}  // namespace

int main() {
  size_t blk = 1, ncv = 0, nev = 0, hr = 0, hcn = 0;
  HMat H;
  std::string cmd;
  while (std::cin >> cmd) {
    std::printf("{\"cmd\": \"%s\", ", cmd.c_str());
    if (cmd == "consts") {
      std::printf("\"KS_AGREE\": %d, \"slots\": [%d,%d,%d], \"MB_R\": %zu, \"MB_COEF\": %zu", KS_AGREE, KS_AGREE_MAX_RANK, KS_AGREE_NEG_MIN_RANK, KS_AGREE_STATUS, KS_MB_R, KS_MB_COEF);
    } else if (cmd == "args") {
      int nev_, ncv_, blk_, maxit;
      unsigned long long dim;
      std::cin >> nev_ >> ncv_ >> blk_ >> maxit >> dim;
      const size_t b = ks_effective_blk(nev_, blk_);
      std::printf("\"blk\": %zu, \"counts\": %d, \"range\": %d", b, (int)ks_check_counts(nev_, blk_, maxit), (int)ks_check_range(nev_, ncv_, b, dim));
    } else if (cmd == "passes") {
      std::string t;
      std::cin >> t;
      std::printf("\"npass\": %d", ks_ortho_passes(t == "-" ? nullptr : t.c_str()));
    } else if (cmd == "mail") {
      size_t cap_r, b, m;
      int npass;
      std::cin >> cap_r >> b >> npass >> m;
      std::printf("\"floats\": %zu, \"copied\": %zu", ks_mail_floats(cap_r, b), ks_mail_copied(npass, m, b));
    } else if (cmd == "slice") {
      unsigned long long dim;
      int world;
      std::cin >> dim >> world;
      std::printf("\"slices\": [");
      for (int r = 0; r < world; ++r) {
        const KsSlice s = ks_row_slice(dim, world, r);
        std::printf("%s[%llu,%llu,%llu]", r ? "," : "", (unsigned long long)s.nloc, (unsigned long long)s.r0, (unsigned long long)s.r1);
      }
      std::printf("]");
    } else if (cmd == "stage") {
      size_t n, keep, nconv;
      std::cin >> n >> keep >> nconv;
      const KsStage s = ks_stage_layout(n, keep, nconv);
      std::printf("\"subH\": %zu, \"vH\": %zu, \"blkH\": %zu, \"top\": %zu, \"bytes\": %zu", s.subH, s.vH, s.blkH, s.top, s.bytes);
    } else if (cmd == "blk" || cmd == "ncv" || cmd == "nev") {
      size_t& v = cmd == "blk" ? blk : cmd == "ncv" ? ncv : nev;
      std::cin >> v;
      std::printf("\"value\": %zu", v);
    } else if (cmd == "tight") {
      size_t r, c;
      std::cin >> r >> c;
      H = HMat(r, c);
      H.a = take(r * c);
      put(H);
    } else if (cmd == "start") {
      int rank;
      std::cin >> rank;
      const std::vector<float> hc = take(2 * blk * blk), R = take((size_t)rank * blk);
      H = ks_h_start(blk, ncv, hc.data(), R.data(), rank);
      put(H);
    } else if (cmd == "reserve") {
      const KsCap cap = ks_h_reserve(H, ncv, blk);
      hr = H.r;
      hcn = H.c;
      std::printf("\"ask_r\": %zu, \"ask_c\": %zu, ", cap.r, cap.c);
      put(H);
    } else if (cmd == "fold") {
      int npass, rk;
      std::cin >> npass >> rk;
      const std::vector<float> hc = take((size_t)npass * hr * blk), R = take((size_t)rk * blk);
      ks_fold_step(H, hr, hcn, blk, npass, hc.data(), R.data(), rk);
      H.r = hr += blk;
      H.c = hcn += blk;
      put(H);
    } else if (cmd == "truncate") {
      size_t nconv;
      std::cin >> nconv;
      const size_t n = H.c - nconv, keep = nev - nconv;
      const std::vector<float> eH = take(n), vH = take(n * keep), top = take(nconv * keep);
      std::vector<float> subH(n * n), blkH(nconv * n);  // exactly the sizes of the staging layout: an overrun is the sanitizer's to find
      ks_h_extract_sub(H, nconv, subH.data());
      if (nconv > 0) ks_h_extract_locked(H, nconv, blkH.data());
      H = ks_h_truncate(H, nev, ncv, blk, nconv, eH.data(), vH.data(), top.data());
      put("subH", subH.data(), subH.size());
      std::printf(", ");
      put("blkH", blkH.data(), blkH.size());
      std::printf(", ");
      put(H);
    } else if (cmd == "unconv") {
      float tol;
      int divide;
      std::cin >> tol >> divide;
      std::printf("\"j\": %zu", ks_first_unconverged(H, blk, tol, divide != 0));
    } else if (cmd == "counts") {
      float tol;
      size_t nconv, last_j, n_restarts;
      int maxit;
      std::cin >> tol >> nconv >> last_j >> n_restarts >> maxit;
      const KsCounts k = ks_final_counts(H, blk, tol, nconv, last_j, n_restarts, maxit, (int)nev);
      std::printf("\"nc\": %zu, \"nc_ref\": %zu, \"noconv\": %s", k.nc, k.nc_ref, k.noconv ? "true" : "false");
    } else {
      std::fprintf(stderr, "ks_host_main: unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::printf("}\n");
    if (!std::cin) {
      std::fprintf(stderr, "ks_host_main: %s: input ended or did not parse\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
