// isle_amd/csrc/api_ks.cpp — the restarted block Krylov-Schur solver behind isle_hip_block_ks / isle_hip_block_ks_dense
// (BlockKs::init / expand / truncate / compute, block-ks/restarted_block_ks.h:62-321; compute_qr, block-ks/ks_utils.h:43-127; the glue of
// src/sparseMatrix.cpp:1195-1240).  The host keeps the small projected matrix H and the restart logic; everything V-sized runs in dense.hip /
// evd_tridiag.hip / gram_lds.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "api_internal.h"
#include "ks_host.h"

__global__ void ks_agree_pack_k(int* meta) {
  if (threadIdx.x == 0) {
    meta[KS_AGREE_MAX_RANK] = meta[0];
    meta[KS_AGREE_NEG_MIN_RANK] = -meta[0];
    meta[KS_AGREE_STATUS] = meta[1];
  }
}

// ------------------------------------------------------------------------------------------
// Panel QR: rank-revealing CholQR2 on an fp64 Gram matrix.
// utils::compute_qr (block-ks/ks_utils.h:43-127) is MGS in double with one DGKS correction and drops
// columns whose residual norm is < 1e-6.  Cholesky of G = F^T F processed column by column IS that MGS
// in exact arithmetic (pivot_i^2 = residual norm^2 of column i); a second pass restores orthogonality
// to working precision.  F: n x w (device, destroyed).  Q: n x rank written to Qdst.  R: rank x w.
// ------------------------------------------------------------------------------------------
static int dev_qr(isle_ctx* c, float* F, uint64_t n, int w, float* Qdst, std::vector<float>& R, int* rank_out) {
  std::vector<float> Rfull((size_t)w * w, 0.f);
  int rk = 0;
  ISLECHK(k_panel_qr(c, F, n, w, Qdst, Rfull.data(), &rk));
  ISLECHK(agree_i32(c, rk, "the rank of a start / repair block"));
  *rank_out = rk;
  R.assign(Rfull.begin(), Rfull.begin() + (size_t)rk * w);
  return 0;
}

// ------------------------------------------------------------------------------------------
// Restarted block Krylov-Schur
// ------------------------------------------------------------------------------------------
namespace {
struct Ks {
  isle_ctx* c;
  size_t nev, ncv, maxit, blk;
  uint64_t dim;
  float tol;
  HMat H;
  size_t vcols = 0, nconv = 0, n_restarts = 0, last_j = 0;
  long napplies = 0;
  uint64_t seed, draws = 0;
  // The ProdOp plug-in (block-ks/restarted_block_ks.h:18-40): the context's B B^T (MKL_SpSpTrProd, include/matUtils.h:336-365), or a
  // dense symmetric dim x dim matrix on the device (ArmaMatProdOp, block-ks/ks_utils.h:167-182) when dense_A is set.
  const float* dense_A = nullptr;
  const float* start_dev = nullptr;  // optional dim x blk start block (first try of init's draw loop)
  float* Vb() { return c->basis.p; }
  float* col(size_t j) { return c->basis.p + j * dim; }

  int randu(float* F, size_t cols) { return k_randu(c, F, dim * cols, seed + 0x1000 * (++draws)); }

  // orthogonalise F (dim x w) against the first m basis columns, `passes` times; coefficient blocks kept on device
  int ortho(float* F, int w, size_t m, int passes, float* coef_dev = nullptr) {
    HIPCHK(c, c->coef.reserve(3 * (c->basis.cap / dim) * 32));
    float* base = coef_dev ? coef_dev : c->coef.p;
    // Several ranks: the basis is replicated, but nobody needs to orthogonalise ALL rows.  Rank r takes rows [r nloc, (r+1) nloc):
    // its share of V^T F, an all-reduce of the m x w coefficients (80 kB at m = 2000), the update of its rows — for every pass —
    // and at the end the slices of F are all-gathered (4 MB at V = 100k), so every rank again holds the whole, bitwise equal F for
    // the replicated panel QR.  The step is HBM-bound on reading the basis (0.15 s of a 1.15 s C3-shard step): it now divides by
    // the number of ranks at the price of passes + 1 small collectives per step.  Default with several ranks since round 5 (a collective
    // that never completes is turned into ISLE_E_COMM by the watchdog, api.cpp); ISLE_KS_ROWSHARD=0 keeps it replicated.
    const bool shard = route_ks_rowshard(c->multi(), dense_A, c->route);
    if (!shard) {
      for (int p = 0; p < passes; ++p) {
        float* cf = base + (size_t)p * m * w;
        ISLECHK(k_vtf(c, Vb(), dim, (int)m, F, w, cf));
        ISLECHK(k_update(c, F, dim, w, Vb(), (int)m, cf));
      }
      return 0;
    }
    const KsSlice my = ks_row_slice(dim, c->world, c->rank);
    const uint64_t nloc = my.nloc, r0 = my.r0, nl = my.r1 - my.r0;
    for (int p = 0; p < passes; ++p) {
      float* cf = base + (size_t)p * m * w;
      ISLECHK(k_vtf(c, Vb() + r0, nl, (int)m, F + r0, w, cf, dim));
      ISLECHK(allreduce_sum<float>(c, cf, m * (size_t)w));
      ISLECHK(k_update(c, F + r0, nl, w, Vb() + r0, (int)m, cf, dim));
    }
    HIPCHK(c, c->ks_gather.reserve((size_t)c->world * nloc * w));
    float* mine = c->ks_gather.p + (size_t)c->rank * nloc * w;
    ISLECHK(k_slice_rows(c, F, dim, w, r0, nl, nloc, mine, true));  // pack my rows (zero padded to nloc)
    {
      TimeScope ts(c, ISLE_T_COMM);
      ISLECHK(isle_allgather(c, mine, c->ks_gather.p, nloc * (size_t)w, ISLE_DT_F32));
    }
    for (int r = 0; r < c->world; ++r) {
      const KsSlice q = ks_row_slice(dim, c->world, r);
      if (r != c->rank && q.r1 > q.r0) ISLECHK(k_slice_rows(c, F, dim, w, q.r0, q.r1 - q.r0, nloc, c->ks_gather.p + (size_t)r * nloc * w, false));
    }
    return 0;
  }

  // rank repair shared by init (:238-258) and expand (:106-132)
  int repair(size_t& nvecs, size_t target, size_t width) {
    size_t tries = 0;
    while (nvecs < target && tries < 100) {
      tries++;
      ISLECHK(randu(c->Fbuf.p, width));
      ISLECHK(ortho(c->Fbuf.p, (int)width, nvecs, 2));
      std::vector<float> R2;
      int rk2 = 0;
      const size_t room = target - nvecs;
      // Q lands in Tmp first: only `room` columns may be appended
      ISLECHK(dev_qr(c, c->Fbuf.p, dim, (int)width, c->Tmp.p, R2, &rk2));
      const size_t take = std::min<size_t>((size_t)rk2, room);
      if (take) HIPCHK(c, hipMemcpyAsync(col(nvecs), c->Tmp.p, take * dim * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      nvecs += take;
    }
    if (nvecs < target) return isle_fail(c, ISLE_E_NUMERIC, "unable to find new starting basis for Arnoldi expansion");
    return 0;
  }

  int apply(const float* X, float* Z) {
    napplies++;
    if (dense_A) return k_gemm_nn(c, dense_A, dim, (int)dim, X, (int)dim, (int)blk, Z, ISLE_T_GRAM_PASS1);
    return gram_apply_dev(c, X, (int)blk, Z);
  }

  int init() {  // :203-259
    std::vector<float> R;
    int rank = 0;
    bool first = true;
    do {  // :211-218: redrawn until the start block has full rank
      if (first && start_dev) HIPCHK(c, hipMemcpyAsync(c->Fbuf.p, start_dev, dim * blk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      else ISLECHK(randu(c->Fbuf.p, blk));
      first = false;
      ISLECHK(dev_qr(c, c->Fbuf.p, dim, (int)blk, col(0), R, &rank));
    } while ((size_t)rank < blk);
    float* V1 = c->Fbuf.p;
    ISLECHK(apply(col(0), V1));
    ISLECHK(ortho(V1, (int)blk, blk, 2));  // H = V^T V1; V1 -= V H; C = V^T V1; H += C; V1 -= V C
    std::vector<float> hc(2 * blk * blk);
    HIPCHK(c, hipMemcpyAsync(hc.data(), c->coef.p, hc.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    ISLECHK(dev_qr(c, V1, dim, (int)blk, col(blk), R, &rank));  // synchronises the stream
    H = ks_h_start(blk, ncv, hc.data(), R.data(), rank);
    vcols = blk + rank;
    if ((size_t)rank < blk) ISLECHK(repair(vcols, 2 * blk, blk - rank));
    vcols = 2 * blk;
    return 0;
  }

  // ---- expand (:62-136) --------------------------------------------------------------------------------------------------------------------
  // Pipelined: after the QR of step i is enqueued, the operator application and orthogonalisation of step i + 1 are
  // enqueued too (they only need Q on the device, assuming full rank), and the host then waits for an event recorded
  // behind the QR to fold R and the coefficients into H.  Everything the host needs from a step — rank and status of the QR,
  // R, the three coefficient blocks — is written into one device mailbox (ks_host.h) and comes back as ONE copy (every small copy
  // costs ~20 us of queue time).  A rank-deficient panel (never seen on thresholded matrices) discards the speculative
  // work and repairs, as the synchronous form (ISLE_KS_SYNC=1) does.
  // Round 6: the copy runs on a stream of its own behind an event — in the main stream it held the next step's kernels back for the ~10 us
  // a 160 kB transfer over PCIe takes, 300 times per solve — and the device mailbox is double-buffered by slot, so that the next step's
  // coefficients (written by the speculative orthogonalisation) never land in a mailbox whose copy may still be reading it: a slot is
  // written again only after the host has waited for its copy.
  struct Expand {
    KsCap cap;              // rows / columns the work matrix has room for
    int npass;              // passes of block Gram-Schmidt per step (2, or 3 under ISLE_KS_ORTHO_PASSES)
    bool pipelined;         // step i + 1 is enqueued before the host waits for step i (not under ISLE_KS_SYNC)
    float* mail[2];         // the two device mailboxes
    float* host_mail[2];    // where their copies land: page-locked when they fit the context's slots, else host_mail_pageable
    std::vector<float> host_mail_pageable[2];
    size_t hr, hcn;         // rows / columns of H written so far; H.r / H.c take them in shrink()
    bool spec = false;      // apply + ortho of the step that comes next are already enqueued, into mailbox `slot`
    int slot = 0;           // mailbox, landing area and events of the current step; a speculative step writes the other one
  };

  // mailboxes, events, the copy stream and the host landing slots
  int expand_prepare(Expand& e) {
    e.pipelined = route_ks_pipelined(c->route);
    e.npass = c->route.ks_ortho_passes;
    const size_t mb_floats = ks_mail_floats(e.cap.r, blk);
    HIPCHK(c, c->ks_mail.reserve(2 * mb_floats));
    for (int i = 0; i < 2; ++i) {
      if (!c->ks_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ks_ev[i], hipEventDisableTiming));
      if (!c->ks_ev_ready[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ks_ev_ready[i], hipEventDisableTiming));
    }
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      if (mb_floats * sizeof(float) <= isle_ctx::PIN_MAIL_SLOT) {  // page-locked: the copy of qr_and_post then really is asynchronous
        e.host_mail[i] = reinterpret_cast<float*>(c->pin + isle_ctx::PIN_MAIL + (size_t)i * isle_ctx::PIN_MAIL_SLOT);
      } else {
        e.host_mail_pageable[i].resize(mb_floats);
        e.host_mail[i] = e.host_mail_pageable[i].data();
      }
      e.mail[i] = c->ks_mail.p + (size_t)i * mb_floats;
    }
    return 0;
  }

  // operator application to basis columns [from_col, from_col + blk) and orthogonalisation against the first m basis vectors, the
  // coefficients into `mailbox`: the step itself, or the speculative next one
  int enqueue_step(const Expand& e, size_t m, size_t from_col, float* mailbox) {
    ISLECHK(apply(col(from_col), c->Fbuf.p));
    return ortho(c->Fbuf.p, (int)blk, m, e.npass, mailbox + KS_MB_COEF);
  }

  // panel QR of the step into basis columns [hcn + blk, ..), the ranks' agreement on it, and the mailbox's copy to the host posted on the copy stream
  int qr_and_post(const Expand& e, size_t m) {
    float* mail = e.mail[e.slot];
    ISLECHK(k_panel_qr_kernels(c, c->Fbuf.p, dim, (int)blk, col(e.hcn + blk), reinterpret_cast<int*>(mail), mail + KS_MB_R));
    if (c->multi()) {  // the ranks' verdicts on this block travel with the mailbox (see agree_i32)
      hipLaunchKernelGGL(ks_agree_pack_k, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<int*>(mail));
      HIPCHK(c, hipGetLastError());
      TimeScope ts(c, ISLE_T_COMM);
      ISLECHK(isle_allreduce(c, reinterpret_cast<int*>(mail) + KS_AGREE, 3, ISLE_DT_I32, true));
    }
    HIPCHK(c, hipEventRecord(c->ks_ev_ready[e.slot], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ks_ev_ready[e.slot], 0));
    HIPCHK(c, hipMemcpyAsync(e.host_mail[e.slot], mail, ks_mail_copied(e.npass, m, blk) * sizeof(float), hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipEventRecord(c->ks_ev[e.slot], c->copy_stream));
    return 0;
  }

  // the step's mailbox has landed: the two failure verdicts, else the rank of its panel
  int wait_and_check(const Expand& e, int* rk) {
    HIPCHK(c, hipEventSynchronize(c->ks_ev[e.slot]));
    const int* meta = reinterpret_cast<const int*>(e.host_mail[e.slot]);
    if (c->multi() && meta[KS_AGREE_MAX_RANK] != -meta[KS_AGREE_NEG_MIN_RANK])
      return isle_fail(c, ISLE_E_COMM, "ranks disagree on the rank of a Krylov block (min %d, max %d): replicated state diverged",
                       -meta[KS_AGREE_NEG_MIN_RANK], meta[KS_AGREE_MAX_RANK]);
    if (meta[1] || (c->multi() && meta[KS_AGREE_STATUS]))
      return isle_fail(c, ISLE_E_NUMERIC, "CholQR2: second Gram matrix not positive definite");
    *rk = meta[0];
    return 0;
  }

  void shrink(const Expand& e) {
    H.r = e.hr;
    H.c = e.hcn;
  }

  // a panel of rank rk < blk: the speculative step used columns that are about to be replaced
  int repair_after(Expand& e, int rk) {
    if (e.spec) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      e.spec = false;
      napplies--;
    }
    shrink(e);  // repair() reads H.r / H.c
    size_t nvecs = H.c + rk;
    return repair(nvecs, H.r, blk - rk);
  }

  int expand() {
    isle_host_mark("expand: entry");
    Expand e;
    e.cap = ks_h_reserve(H, ncv, blk);  // H grows in place: rows hr.. and columns hcn.. are zero until a step writes them
    e.hr = H.r;
    e.hcn = H.c;
    ISLECHK(expand_prepare(e));
    isle_host_mark("expand: work matrix ready");
    while (e.hr < ncv) {
      const size_t m = e.hr;
      if (!e.spec) ISLECHK(enqueue_step(e, m, e.hcn, e.mail[e.slot]));
      e.spec = false;
      if (m + blk > e.cap.r || e.hcn + blk > e.cap.c) return isle_fail(c, ISLE_E_NUMERIC, "expand: projected matrix outgrew its work space");
      ISLECHK(qr_and_post(e, m));
      if (e.pipelined && m + blk < ncv) {  // speculate: full rank -> next step works on the blk new columns with m + blk basis vectors
        ISLECHK(enqueue_step(e, m + blk, e.hcn + blk, e.mail[e.slot ^ 1]));  // the other slot's mailbox: its last copy has been waited for
        e.spec = true;
      }
      int rk = 0;
      ISLECHK(wait_and_check(e, &rk));
      ks_fold_step(H, m, e.hcn, blk, e.npass, e.host_mail[e.slot] + KS_MB_COEF, e.host_mail[e.slot] + KS_MB_R, rk);
      e.hr = m + blk;
      e.hcn += blk;
      if ((size_t)rk < blk) ISLECHK(repair_after(e, rk));
      e.slot ^= 1;
    }
    isle_host_mark("expand: loop done");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    isle_host_mark("expand: synchronised");
    shrink(e);
    isle_host_mark("expand: shrink");
    vcols = H.r;
    return 0;
  }

  // ---- truncate (:138-187) -----------------------------------------------------------------------------------------------------------------
  // Everything that crosses the bus here lives in the context's page-locked staging area (ks_stage_layout): copies from freshly
  // allocated pageable vectors blocked the host (registration with the driver) and made their release slow, with the GPU idle in between.
  struct Stage {
    float *subH, *vH, *blkH, *top;
  };

  // V = [ V(:, :nconv) | V(:, nconv : ncols-blk) * vH(:, :keep) | V(:, tail blk) ] with the Ritz rotation in Wf (n x keep); vH and,
  // with locked pairs, top come back to the staging area.  Ends synchronised.
  int rotate_basis(const Stage& st, size_t n, size_t keep) {
    HIPCHK(c, hipMemcpyAsync(st.vH, c->Wf.p, n * keep * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    ISLECHK(k_gemm_nn(c, col(nconv), dim, (int)n, c->Wf.p, (int)n, (int)keep, c->Tmp.p));
    // top = H(0:nconv, nconv:) * vH(:, :keep)  (:176-178), the coupling of the locked columns with the rotated block: nconv x n x keep
    // multiply-adds — 0.3 G at k = 1000 with 600 pairs locked, 31 ms of host time with the GPU idle when it was a host loop
    if (nconv > 0) {
      HIPCHK(c, c->ks_top.reserve(nconv * n + nconv * keep));
      ks_h_extract_locked(H, nconv, st.blkH);
      HIPCHK(c, hipMemcpyAsync(c->ks_top.p, st.blkH, nconv * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
      ISLECHK(k_gemm_nn(c, c->ks_top.p, nconv, (int)n, c->Wf.p, (int)n, (int)keep, c->ks_top.p + nconv * n));
      HIPCHK(c, hipMemcpyAsync(st.top, c->ks_top.p + nconv * n, nconv * keep * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->Fbuf.p, col(vcols - blk), blk * dim * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(col(nconv), c->Tmp.p, keep * dim * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(col(nev), c->Fbuf.p, blk * dim * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    vcols = nev + blk;
    return 0;
  }

  int truncate() {
    isle_host_mark("truncate: entry");
    const size_t n = H.c - nconv;
    const size_t keep = nev - nconv;  // only the leading `keep` eigenvectors are used below
    const KsStage lay = ks_stage_layout(n, keep, nconv);
    HIPCHK(c, c->pin_stage.reserve(lay.bytes));
    float* base = reinterpret_cast<float*>(c->pin_stage.p);
    const Stage st{base + lay.subH, base + lay.vH, base + lay.blkH, base + lay.top};
    ks_h_extract_sub(H, nconv, st.subH);
    isle_host_mark("truncate: subH extracted");
    std::vector<float> eH(n);
    HIPCHK(c, c->Wf.reserve(n * n));
    ISLECHK(k_eig_small(c, st.subH, (int)n, eH.data(), c->Wf.p, (int)keep));
    isle_host_mark("truncate: eig_small returned");
    ISLECHK(rotate_basis(st, n, keep));
    isle_host_mark("truncate: device part synchronised");
    H = ks_h_truncate(H, nev, ncv, blk, nconv, eH.data(), st.vH, st.top);
    isle_host_mark("truncate: H transformed");
    return 0;
  }

  int compute() {  // :261-321
    n_restarts = 0;
    nconv = 0;
    ISLECHK(expand());
    while (n_restarts < maxit) {
      ISLECHK(truncate());
      const size_t j = ks_first_unconverged(H, blk, tol, true);  // :278-293
      ISLECHK(agree_i32(c, (int)j, "the number of converged Ritz pairs"));
      last_j = j;
      if (j == H.c) {
        nconv = H.c;
        break;
      }
      nconv = j;
      ++n_restarts;
      ISLECHK(expand());
    }
    return 0;
  }
};
}  // namespace

int install_U(isle_ctx* c, const float* Ucm_dev, int k) {
  c->ldk = round4(k);
  HIPCHK(c, c->Ucm.reserve((size_t)c->V * k));
  HIPCHK(c, c->Urm.reserve((size_t)c->V * c->ldk));
  if (Ucm_dev != c->Ucm.p)
    HIPCHK(c, hipMemcpyAsync(c->Ucm.p, Ucm_dev, (size_t)c->V * k * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->Urm.p, 0, (size_t)c->V * c->ldk * sizeof(float), c->stream));
  ISLECHK(k_transpose(c, c->Ucm.p, c->V, k, c->V, c->Urm.p, c->ldk));  // compute_U_rowmajor :1223-1231
  c->res.U_installed(k);
  return 0;
}

// Shared driver of both eigensolver entries: BlockKs(op, nev, ncv, maxit, blk, tol); init(); compute()  (:190-321).
// ncv and nev need not be multiples of the block size: a decomposition grows by whole blocks until it has AT LEAST ncv
// rows (the reference sizes V for exactly ncv columns and overruns it in that case), so the basis holds up to
// ncv + blk - 1 vectors.
static int ks_solve(isle_ctx* c, Ks& ks, int nev, int ncv, int maxit, int blk, float tol, uint64_t seed, float* evals, int* nconv,
                    int* restarts, int* napplies, int* nconv_ref_rule) {
  if (ks_check_counts(nev, blk, maxit) != KS_ARGS_OK) return isle_fail(c, ISLE_E_ARG, "bad nev/blk/maxit (nev >= 1, 1 <= blk <= 32, maxit >= 1)");
  ks.c = c;
  ks.nev = nev;
  ks.ncv = ncv;
  ks.maxit = maxit;
  ks.blk = ks_effective_blk(nev, blk);
  ks.tol = tol;
  ks.seed = seed;
  if (ks_check_range(nev, ncv, ks.blk, ks.dim) != KS_ARGS_OK)
    return isle_fail(c, ISLE_E_ARG, "need nev + 2*blk <= ncv and ncv + blk <= operator dimension (nev=%d ncv=%d blk=%zu dim=%llu)", nev, ncv,
                     ks.blk, (unsigned long long)ks.dim);
  HIPCHK(c, c->basis.reserve((size_t)ks.dim * (ncv + 2 * ks.blk)));
  HIPCHK(c, c->Fbuf.reserve((size_t)ks.dim * ks.blk));
  HIPCHK(c, c->Tmp.reserve((size_t)ks.dim * std::max<size_t>(nev, ks.blk)));
  isle_host_mark("ks_solve: entry");
  ISLECHK(ks.init());
  isle_host_mark("ks_solve: init done");
  ISLECHK(ks.compute());
  isle_host_mark("ks_solve: compute done");
  const KsCounts k = ks_final_counts(ks.H, ks.blk, ks.tol, ks.nconv, ks.last_j, ks.n_restarts, maxit, nev);
  const int rc = k.noconv ? ISLE_E_NOCONV : 0;
  const size_t nc = k.nc, nc_ref = k.nc_ref;
  for (int i = 0; i < nev; ++i) evals[i] = ks.H(i, i);  // src/sparseMatrix.cpp:1212-1213
  if (nconv) *nconv = (int)nc;
  if (nconv_ref_rule) *nconv_ref_rule = (int)nc_ref;
  if (restarts) *restarts = (int)ks.n_restarts;
  if (napplies) *napplies = (int)ks.napplies;
  return rc;
}

extern "C" int isle_hip_block_ks(isle_ctx* c, int nev, int ncv, int maxit, int blk, float tol, uint64_t seed, float* evals, int* nconv,
                                 int* restarts, int* napplies) {
  if (!c || !evals) return ISLE_E_ARG;
  if (c->V == 0) return isle_fail(c, ISLE_E_ARG, "no matrix uploaded");
  ISLECHK(isle_enter(c));
  Ks ks;
  ks.dim = c->V;
  c->res.operator_must_be_rebuilt();  // the operator (CSR copy) is rebuilt per solve, as in src/sparseMatrix.cpp:1199
  int nc = 0;
  const int rc = ks_solve(c, ks, nev, ncv, maxit, blk, tol, seed, evals, &nc, restarts, napplies, nullptr);
  if (nconv) *nconv = nc;
  if (rc != 0 && rc != ISLE_E_NOCONV) return rc;
  ISLECHK(install_U(c, c->basis.p, nev));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  isle_host_mark("block_ks: U installed, exit");
  if (rc == ISLE_E_NOCONV) return isle_fail(c, rc, "block KS: %d restarts exhausted, %d of %d Ritz pairs converged", maxit, nc, nev);
  return 0;
}

extern "C" int isle_hip_block_ks_dense(isle_ctx* c, const float* A, uint64_t n, int nev, int ncv, int maxit, int blk, float tol,
                                       uint64_t seed, const float* start_block, float* evals, float* U, int* nconv, int* nconv_ref_rule,
                                       int* restarts, int* napplies) {
  if (!c || !A || !evals || n < 2 || n > 46340) return isle_fail(c, ISLE_E_ARG, "block_ks_dense: bad arguments (2 <= n <= 46340)");
  ISLECHK(isle_enter(c));
  if (c->multi()) return isle_fail(c, ISLE_E_ARG, "block_ks_dense: the dense operator is not sharded (single rank only)");
  const int b_eff = (int)ks_effective_blk(nev, blk);
  DevBuf<float> Adev, Sdev;
  HIPCHK(c, Adev.reserve((size_t)n * n));
  HIPCHK(c, hipMemcpy(Adev.p, A, (size_t)n * n * sizeof(float), hipMemcpyHostToDevice));
  Ks ks;
  ks.dim = n;
  ks.dense_A = Adev.p;
  if (start_block && b_eff >= 1) {
    HIPCHK(c, Sdev.reserve((size_t)n * b_eff));
    HIPCHK(c, hipMemcpy(Sdev.p, start_block, (size_t)n * b_eff * sizeof(float), hipMemcpyHostToDevice));
    ks.start_dev = Sdev.p;
  }
  int nc = 0;
  const int rc = ks_solve(c, ks, nev, ncv, maxit, blk, tol, seed, evals, &nc, restarts, napplies, nconv_ref_rule);
  if (nconv) *nconv = nc;
  hipError_t he = hipStreamSynchronize(c->stream);
  if (he == hipSuccess && (rc == 0 || rc == ISLE_E_NOCONV) && U)
    he = hipMemcpy(U, c->basis.p, (size_t)n * nev * sizeof(float), hipMemcpyDeviceToHost);
  HIPCHK(c, he);
  if (rc == ISLE_E_NOCONV) return isle_fail(c, rc, "block KS (dense operator): %d restarts exhausted, %d of %d Ritz pairs converged", maxit, nc, nev);
  return rc;
}

extern "C" int isle_hip_get_U(isle_ctx* c, float* U) {
  if (!c || !U || c->res.U_k == 0) return isle_fail(c, ISLE_E_ARG, "no U available");
  ISLECHK(isle_enter(c));
  HIPCHK(c, hipMemcpyAsync(U, c->Ucm.p, (size_t)c->V * c->res.U_k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int isle_hip_set_U(isle_ctx* c, const float* U, int k) {
  if (!c || !U || k < 1 || c->V == 0) return isle_fail(c, ISLE_E_ARG, "set_U: bad arguments");
  ISLECHK(isle_enter(c));
  HIPCHK(c, c->Ucm.reserve((size_t)c->V * k));
  HIPCHK(c, hipMemcpy(c->Ucm.p, U, (size_t)c->V * k * sizeof(float), hipMemcpyHostToDevice));
  ISLECHK(install_U(c, c->Ucm.p, k));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// LAPACK 'U' semantics: the upper triangle is the matrix.  A non-finite entry there would come back as rc 0 with NaN pairs from the
// tridiagonal solver (its Sturm counts and its check compare with NaN): refused here, before any launch.  The strict lower triangle is not read.
static int eig_sym_entry(isle_ctx* c, const float* S, int n, int nvec, float* evals, float* vecs) {
  if (!c || !S || !evals || !vecs || n < 1 || nvec < 1 || nvec > n) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  for (int j = 0; j < n; ++j)
    for (int i = 0; i <= j; ++i)
      if (!std::isfinite(S[(size_t)j * n + i])) return isle_fail(c, ISLE_E_NUMERIC, "eig_sym: entry (%d, %d) of the upper triangle is not finite", i, j);
  HIPCHK(c, c->Wf.reserve((size_t)n * n));  // n x n whatever nvec: the Jacobi solver returns every vector
  ISLECHK(k_eig_small(c, S, n, evals, c->Wf.p, nvec));
  HIPCHK(c, hipMemcpy(vecs, c->Wf.p, (size_t)n * nvec * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int isle_hip_eig_sym(isle_ctx* c, const float* S, int n, float* evals, float* vecs) { return eig_sym_entry(c, S, n, n, evals, vecs); }
extern "C" int isle_hip_eig_sym_leading(isle_ctx* c, const float* S, int n, int nvec, float* evals, float* vecs) {
  return eig_sym_entry(c, S, n, nvec, evals, vecs);
}
extern "C" int isle_hip_eig_info(isle_ctx* c, int* info, float* defect) {
  if (!c || !info) return ISLE_E_ARG;
  for (int i = 0; i < ISLE_EIG_INFO_COUNT; ++i) info[i] = c->eig_info[i];
  if (defect) *defect = c->eig_defect;
  return 0;
}

