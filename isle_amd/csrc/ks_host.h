// isle_amd/csrc/ks_host.h — what the restarted block Krylov-Schur solver (api_ks.cpp) computes on the host: the small projected matrix H and
// every operation on it, the restart counts, the layout of the expand mailbox and of the truncation's staging area, the row slice of a rank
// in the sharded orthogonalisation and the argument rule.  Plain C++ (no HIP type, no isle_ctx, nothing read from the environment), so that
// index arithmetic whose mistakes do not fault but return plausible eigenvalues runs without a device: ks_host_main.cpp replays a case,
// tests/test_ks_host_cpu.py checks it.  The float operation order is the solver's: it is written as measured, and no build of it takes
// -ffast-math, -march or an FMA-enabling flag.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

struct HMat {  // small col-major float matrix on the host (the projected matrix H)
  size_t r = 0, c = 0, ld = 0, cap_c = 0;  // r x c in use inside an ld x cap_c allocation (zero outside what was written)
  std::vector<float> a;
  HMat() {}
  HMat(size_t r_, size_t c_) : r(r_), c(c_), ld(r_), cap_c(c_), a(r_ * c_, 0.f) {}
  // room to grow: the Krylov expansion appends blocks of rows and columns in place (at ncv = 2010 the matrix is 16 MB, and every
  // fresh copy of it cost the host 2 - 6 ms with the GPU idle)
  HMat(size_t r_, size_t c_, size_t cap_r_, size_t cap_c_) : r(r_), c(c_), ld(std::max(r_, cap_r_)), cap_c(std::max(c_, cap_c_)), a(ld * cap_c, 0.f) {}
  float& operator()(size_t i, size_t j) { return a[j * ld + i]; }
  float operator()(size_t i, size_t j) const { return a[j * ld + i]; }
};
inline HMat hsub(const HMat& m, size_t r0, size_t c0, size_t r1, size_t c1) {  // inclusive bounds (arma submat)
  HMat o(r1 - r0 + 1, c1 - c0 + 1);
  for (size_t j = c0; j <= c1; ++j)
    for (size_t i = r0; i <= r1; ++i) o(i - r0, j - c0) = m(i, j);
  return o;
}

// ---- the arguments of a solve -------------------------------------------------------------------------------------------------------------
inline size_t ks_effective_blk(int nev, int blk) {  // block-ks/restarted_block_ks.h:198
  return (blk < nev) ? blk : 1;
}
enum KsArgs { KS_ARGS_OK = 0, KS_ARGS_COUNTS, KS_ARGS_NCV_SMALL, KS_ARGS_NCV_LARGE };
inline KsArgs ks_check_counts(int nev, int blk, int maxit) { return (nev < 1 || blk < 1 || blk > 32 || maxit < 1) ? KS_ARGS_COUNTS : KS_ARGS_OK; }
// blk: the effective width.  ncv and nev need not be multiples of it (see ks_h_reserve)
inline KsArgs ks_check_range(int nev, int ncv, size_t blk, uint64_t dim) {
  if ((size_t)ncv < (size_t)nev + 2 * blk) return KS_ARGS_NCV_SMALL;
  if ((uint64_t)ncv + blk > dim) return KS_ARGS_NCV_LARGE;
  return KS_ARGS_OK;
}
// Passes of block Gram-Schmidt against the basis per step.  The reference makes three (CGS + 2 DGKS, :83-91); the second
// already leaves coefficients at rounding level ("twice is enough"), so two are made here and the third
// block of coefficients that the reference adds into H is zero.  ISLE_KS_ORTHO_PASSES=3 (`asked`, null when unset) restores the
// reference's count.
inline int ks_ortho_passes(const char* asked) {
  int npass = 2;
  if (asked) npass = std::max(2, std::min(3, atoi(asked)));
  return npass;
}

// ---- the expand mailbox: [meta ints | R | coefficients], in floats -------------------------------------------------------------------------
// meta[0] / meta[1]: rank and status of the panel QR; with several ranks the three slots from KS_AGREE on hold what all of them found
constexpr int KS_AGREE = 40;  // int slots [40, 43) of the expand mailbox: max rank, -min rank, max status over all ranks
constexpr int KS_AGREE_MAX_RANK = KS_AGREE, KS_AGREE_NEG_MIN_RANK = KS_AGREE + 1, KS_AGREE_STATUS = KS_AGREE + 2;
constexpr size_t KS_MB_R = 64, KS_MB_COEF = 64 + 32 * 32;  // mailbox offsets (floats): R (up to 32 x 32) and the coefficient blocks
inline size_t ks_mail_floats(size_t cap_r, size_t blk) { return KS_MB_COEF + 3 * cap_r * blk; }  // one mailbox: room for three passes at any m
inline size_t ks_mail_copied(int npass, size_t m, size_t blk) { return KS_MB_COEF + (size_t)npass * m * blk; }  // what a step brings back

// ---- the row slice of a rank in the sharded orthogonalisation ------------------------------------------------------------------------------
struct KsSlice {
  uint64_t nloc;    // rows per rank, a multiple of 4 (16-byte aligned slices); the same for every rank
  uint64_t r0, r1;  // this rank's rows [r0, r1), clipped to dim (empty for the last ranks of a small dim)
};
inline KsSlice ks_row_slice(uint64_t dim, int world, int rank) {
  KsSlice s;
  s.nloc = (((dim + world - 1) / world) + 3) & ~3ull;
  s.r0 = std::min<uint64_t>(dim, (uint64_t)rank * s.nloc);
  s.r1 = std::min<uint64_t>(dim, s.r0 + s.nloc);
  return s;
}

// ---- H after init: the two coefficient blocks hc (2 x blk x blk) of the first step summed, above `rank` rows of R --------------------------
inline HMat ks_h_start(size_t blk, size_t ncv, const float* hc, const float* R, int rank) {
  HMat H(2 * blk, blk, std::max<size_t>(ncv, 2 * blk) + blk, blk + (std::max<size_t>(ncv, 2 * blk) + blk - 2 * blk));  // room for expand (ks_h_reserve)
  for (size_t j = 0; j < blk; ++j) {
    for (size_t i = 0; i < blk; ++i) H(i, j) = hc[j * blk + i] + hc[blk * blk + j * blk + i];
    for (int i = 0; i < rank; ++i) H(blk + i, j) = R[j * rank + i];
  }
  return H;
}

// ---- expand ----------------------------------------------------------------------------------------------------------------------------------
// H grows by blk rows and columns per step; it is kept in a work matrix of the final size while the loop runs (copying
// the whole of H at every step cost ~10 ms of host time per solve at ncv = 410, with the GPU idle behind the QR's sync).
// ncv and nev need not be multiples of the block size: a decomposition grows by whole blocks until it has AT LEAST ncv rows.
struct KsCap {
  size_t r, c;  // rows / columns the expansion may reach
};
inline KsCap ks_h_reserve(HMat& H, size_t ncv, size_t blk) {
  const size_t cap_r = std::max<size_t>(ncv, H.r) + blk, cap_c = H.c + (cap_r - H.r);
  if (H.ld < cap_r || H.cap_c < cap_c) {  // ks_h_start and ks_h_truncate allocate with this room, so this copy is the exception
    HMat W(H.r, H.c, cap_r, cap_c);
    for (size_t j = 0; j < H.c; ++j)
      for (size_t i = 0; i < H.r; ++i) W(i, j) = H(i, j);
    H = std::move(W);
  }
  return KsCap{cap_r, cap_c};
}
// one step folded into columns [hcn, hcn + blk) of the work matrix W, whose rows m.. and columns hcn.. are zero until a step writes them:
// the sum of the npass coefficient blocks hc (each m x blk) in rows [0, m), rk rows of R (rk x blk) below them
inline void ks_fold_step(HMat& W, size_t m, size_t hcn, size_t blk, int npass, const float* hc, const float* Rfull, int rk) {
  for (size_t j = 0; j < blk; ++j)
    for (size_t i = 0; i < m; ++i) {
      float h = hc[j * m + i];
      h = h + hc[m * blk + j * m + i];
      if (npass > 2) h = h + hc[2 * m * blk + j * m + i];
      W(i, hcn + j) = h;
    }
  for (size_t j = 0; j < blk; ++j)
    for (int i = 0; i < rk; ++i) W(m + i, hcn + j) = Rfull[j * rk + i];
}

// ---- truncate --------------------------------------------------------------------------------------------------------------------------------
// The staging area of a truncation with n = H.c - nconv columns in play, of which keep = nev - nconv are rotated:
// [subH n x n | vH n x keep | locked rows of H nconv x n | top nconv x keep], offsets in floats, 36 MB at k = 1000
struct KsStage {
  size_t subH, vH, blkH, top, bytes;
};
inline KsStage ks_stage_layout(size_t n, size_t keep, size_t nconv) {
  KsStage s;
  s.subH = 0;
  s.vH = s.subH + n * n;
  s.blkH = s.vH + n * keep;
  s.top = s.blkH + nconv * n;
  s.bytes = (n * n + n * keep + nconv * n + nconv * keep) * sizeof(float);
  return s;
}
inline void ks_h_extract_sub(const HMat& H, size_t nconv, float* subH) {  // H(nconv:, nconv:), square, n x n packed
  const size_t n = H.c - nconv;
  for (size_t j = 0; j < n; ++j) memcpy(subH + j * n, &H.a[(nconv + j) * H.ld + nconv], n * sizeof(float));
}
inline void ks_h_extract_locked(const HMat& H, size_t nconv, float* blkH) {  // H(0:nconv, nconv:), nconv x n packed
  const size_t n = H.c - nconv;
  for (size_t t = 0; t < n; ++t) memcpy(blkH + t * nconv, &H.a[(nconv + t) * H.ld], nconv * sizeof(float));
}
// Transform H (:169-184): the locked columns stay; column j of the rotated block takes the Ritz value eH[j - nconv] on the diagonal, the
// coupling `top` (nconv x keep) with the locked rows above it, and below row nev the residual rows: the last blk x blk block of H times
// the last blk rows of the Ritz vectors vH (n x keep)
inline HMat ks_h_truncate(const HMat& H, size_t nev, size_t ncv, size_t blk, size_t nconv, const float* eH, const float* vH, const float* top) {
  const size_t n = H.c - nconv, keep = nev - nconv;
  auto vh = [&](size_t i, size_t j) { return vH[j * n + i]; };
  HMat last = hsub(H, H.r - blk, H.c - blk, H.r - 1, H.c - 1);  // blk x blk
  HMat newrows(blk, keep);
  for (size_t j = 0; j < keep; ++j)
    for (size_t t = 0; t < blk; ++t) {
      const float v = vh(n - blk + t, j);
      for (size_t i = 0; i < blk; ++i) newrows(i, j) += last(i, t) * v;
    }
  const size_t grow_r = std::max<size_t>(ncv, nev + blk) + blk;  // what the next ks_h_reserve asks for
  HMat Hn(nev + blk, nev, grow_r, nev + (grow_r - (nev + blk)));
  for (size_t j = 0; j < nconv; ++j) {  // locked columns keep their entries (rows < nev from the old H; residual rows too)
    for (size_t i = 0; i < nev; ++i) Hn(i, j) = H(i, j);
    for (size_t i = 0; i < blk; ++i) Hn(nev + i, j) = H(nev + i, j);
  }
  for (size_t j = nconv; j < nev; ++j) {
    Hn(j, j) = eH[j - nconv];
    for (size_t i = 0; i < blk; ++i) Hn(nev + i, j) = newrows(i, j - nconv);
    for (size_t i = 0; i < nconv; ++i) Hn(i, j) = top[(j - nconv) * nconv + i];
  }
  return Hn;
}

// ---- the residual test and the counts a solve reports ----------------------------------------------------------------------------------------
inline size_t ks_first_unconverged(const HMat& H, size_t blk, float tol, bool divide) {  // :278-293
  for (size_t j = 0; j < H.c; ++j) {
    float s = 0.f;
    for (size_t i = H.r - blk; i < H.r; ++i) s += H(i, j) * H(i, j);
    float nrm = std::sqrt(s);
    if (divide) nrm = nrm / H(j, j);
    if (nrm >= tol) return j;
  }
  return H.c;
}
struct KsCounts {
  size_t nc, nc_ref;  // converged Ritz pairs by this solver's rule and by the reference's
  bool noconv;        // the restarts ran out with fewer than nev pairs converged (ISLE_E_NOCONV)
};
inline KsCounts ks_final_counts(const HMat& H, size_t blk, float tol, size_t nconv, size_t last_j, size_t n_restarts, int maxit, int nev) {
  KsCounts k{nconv, nconv, false};
  if (n_restarts == (size_t)maxit) {
    // The reference recomputes residuals from the EXPANDED H without dividing by the Ritz value (:303-317); the last blk rows of
    // an expanded H are [0 ... 0 R], so that rule reports min(first column of the last block, nev) = nev whatever happened
    // (SURVEY App. C #7).  Here: the count of the last restart's residual test, status ISLE_E_NOCONV, and the same Ritz pairs;
    // the reference's figure is available through nconv_ref_rule.
    k.nc_ref = ks_first_unconverged(H, blk, tol, false);
    k.nc = std::min(last_j, (size_t)nev);
    if (k.nc < (size_t)nev) k.noconv = true;
  }
  k.nc = std::min(k.nc, (size_t)nev);
  k.nc_ref = std::min(k.nc_ref, (size_t)nev);
  return k;
}
