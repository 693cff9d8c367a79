"""The reference's own known-answer recipe against the HIP eigensolver.

BlockKs<ProdOp> takes any symmetric operator (block-ks/restarted_block_ks.h:18-40); the reference ships a dense test
operator (utils::ArmaMatProdOp, block-ks/ks_utils.h:167-182) and seed spectra (utils::get_seed_eigs, :136-165: 1/i,
1/sqrt(i), evenly spaced).  isle_hip_block_ks_dense runs the SAME Ks loop and kernels as isle_hip_block_ks with that
operator, so these tests reach the paths a thresholded corpus never takes on the GPU: rank repair in init() and
expand() (:106-132, :238-258), exact multiplicities, maxit exhaustion (:303-317), ragged nev / ncv.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def seed_matrix(n, kind, seed):
    """A = Q diag(evs) Q^T with evs = utils::get_seed_eigs(n, kind) (ks_utils.h:136-165) and a random orthogonal Q."""
    i = np.arange(1, n + 1, dtype=np.float64)
    evs = {1: 1.0 / i, 2: 1.0 / np.sqrt(i), 3: i / n}[kind]
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    return ((Q * evs) @ Q.T), np.sort(evs)[::-1]


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("n,k", [(300, 20), (1500, 200)])
def test_seed_spectra_are_recovered(hp, kind, n, k):
    """get_seed_eigs spectra (Zipf 1/i, 1/sqrt(i), linear) recovered to 2e-4 by the HIP solver, k = 20 (ncv 50) and k = 200
    (ncv 410: the small EVD at n = 400 in its persistent form, the panel QR, the f32-MFMA rotation)."""
    from oracle.oracle import block_ks_dense
    A, evs = seed_matrix(n, kind, 100 * kind + k)
    A32 = A.astype(np.float32)
    # n = 300, kinds 1 and 2 (the runs that converge, whose counts are compared below): both sides start from the same block (seed 2: every
    # residual estimate the loop reads stays 17 % or more away from tol in the fp64 restatement of tests/ks_certificate.py, so the converged
    # counts do not hinge on rounding).  Kind 3 uses up maxit on either side and keeps each side's own draw.
    S = np.random.default_rng(2).uniform(size=(n, 10)).astype(np.float32) if n == 300 and kind != 3 else None
    r = hp.block_ks_dense(A32, k, start_block=S, allow_noconv=True)
    top = evs[:k]
    assert np.max(np.abs(r["evals"] - top) / top) <= 2e-4
    U = r["U"].astype(np.float64)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 5e-5
    # Ritz residuals against the true matrix (kind 3 at k = 200 exhausts maxit in the reference too: gap 1/n)
    res = np.linalg.norm(A @ U - U * r["evals"].astype(np.float64), axis=0)
    assert res.max() <= (2e-3 if kind == 3 else 5e-4) * top[0]
    if n == 300:  # same control flow as the CPU restatement from the same start block: restart and application counts are equal when both converge
        o = block_ks_dense(A32, k, start_block=S)
        assert np.max(np.abs(r["evals"] - o["evals"]) / top) <= 2e-4
        if r["rc"] == 0 and o["nconv"] == k and o["restarts"] < 100:
            assert r["restarts"] == o["restarts"] and r["napplies"] == o["napplies"]


def test_rank_repair_in_init_and_expand(hp):
    """An operator of rank 15 with blk = 10: A*V0 has rank 10, the next Krylov block only 5 -> expand() must fill the basis
    with random vectors (:106-132); a rank-1 operator trips the repair inside init() (:238-258).  The reference's
    std::runtime_error there is constructed but never thrown; here failure is ISLE_E_NUMERIC."""
    n, k = 400, 12
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((n, 15)))
    lam = np.linspace(3.0, 1.0, 15)
    A = (Q * lam) @ Q.T
    r = hp.block_ks_dense(A.astype(np.float32), k, ncv=40, allow_noconv=True)
    assert np.max(np.abs(r["evals"] - lam[:k]) / lam[:k]) <= 2e-4
    U = r["U"].astype(np.float64)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 5e-5
    # the residual estimate of a decomposition closed by random fill blocks is zero, so the loop stops at once (0 restarts) with
    # vectors as good as fp32 Gram-Schmidt left them: the restated reference algorithm has 1.3e-2 .. 2.2e-2 here
    assert np.linalg.norm(A @ U - U * r["evals"].astype(np.float64), axis=0).max() <= 3e-2
    # rank 1: init()'s second block is entirely random
    q = Q[:, :1]
    A1 = 2.5 * (q @ q.T)
    r1 = hp.block_ks_dense(A1.astype(np.float32), 11, ncv=40, allow_noconv=True)
    assert abs(r1["evals"][0] - 2.5) <= 5e-4 and np.abs(r1["evals"][1:]).max() <= 1e-4
    assert abs(abs(float(r1["U"][:, 0].astype(np.float64) @ q[:, 0])) - 1.0) <= 1e-4


def test_rank_deficient_start_block_is_redrawn(hp):
    """init() redraws the start block while compute_qr reports rank < blk (:211-218): a start block with two equal columns
    and one zero column must give the same spectrum as a healthy one."""
    n, k = 300, 20
    A, evs = seed_matrix(n, 1, 77)
    S = np.random.default_rng(3).uniform(size=(n, 10)).astype(np.float32)
    S[:, 4] = S[:, 2]
    S[:, 7] = 0.0
    r = hp.block_ks_dense(A.astype(np.float32), k, start_block=S, allow_noconv=True)
    assert np.max(np.abs(r["evals"] - evs[:k]) / evs[:k]) <= 2e-4
    good = np.random.default_rng(4).uniform(size=(n, 10)).astype(np.float32)
    r2 = hp.block_ks_dense(A.astype(np.float32), k, start_block=good, allow_noconv=True)
    assert np.max(np.abs(r2["evals"] - evs[:k]) / evs[:k]) <= 2e-4


def test_exact_multiplicities(hp):
    """Eigenvalue 2 with multiplicity 7, then 1 x 9, then a decaying tail (multiplicities within the block size: a block
    Krylov space of width 10 holds at most 10 copies of one eigenvalue, in the reference as here): all copies come back with
    orthonormal vectors (the small EVD takes its Jacobi fallback for exactly repeated Ritz values).  c * identity: every
    Krylov block after the first is zero -> all further basis vectors come from the repair path."""
    from oracle.oracle import block_ks_dense
    n, k = 500, 30
    evs = np.concatenate([np.full(7, 2.0), np.full(9, 1.0), 0.5 / np.arange(1, n - 15)])
    Q, _ = np.linalg.qr(np.random.default_rng(8).standard_normal((n, n)))
    A = (Q * evs) @ Q.T
    r = hp.block_ks_dense(A.astype(np.float32), k, allow_noconv=True)
    o = block_ks_dense(A.astype(np.float32), k)
    assert np.max(np.abs(o["evals"] - evs[:k])) <= 1e-5  # the restated reference algorithm finds them
    assert np.max(np.abs(r["evals"] - evs[:k])) <= 2e-4
    U = r["U"].astype(np.float64)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 5e-5
    assert np.linalg.svd(Q[:, :7].T @ U[:, :7], compute_uv=False).min() >= 1 - 1e-3   # the whole eigenspace of 2
    assert np.linalg.svd(Q[:, 7:16].T @ U[:, 7:16], compute_uv=False).min() >= 1 - 1e-3  # and of 1
    Ai = (3.0 * np.eye(200)).astype(np.float32)
    ri = hp.block_ks_dense(Ai, 20, allow_noconv=True)
    assert np.abs(ri["evals"] - 3.0).max() <= 1e-5
    Ui = ri["U"].astype(np.float64)
    assert np.abs(Ui.T @ Ui - np.eye(20)).max() <= 5e-5


def test_maxit_exhaustion_reports_noconv_with_the_references_rule(hp):
    """maxit restarts used up (:303-317): the reference recomputes residuals from the expanded H without dividing and so
    reports nconv = nev although pairs are unconverged.  The library returns the same last Ritz values,
    status ISLE_E_NOCONV, the honest count in nconv and the reference's figure in nconv_ref_rule; the CPU restatement of the
    reference's rule gives the same figure."""
    from oracle.oracle import block_ks_dense
    n, k = 600, 20
    A, evs = seed_matrix(n, 3, 9)  # evenly spaced: gap 1/n, far from converged after 2 restarts
    A32 = A.astype(np.float32)
    r = hp.block_ks_dense(A32, k, maxit=2, tol=1e-7, allow_noconv=True)
    o = block_ks_dense(A32, k, maxit=2, tol=1e-7)
    assert r["rc"] == -3 and r["restarts"] == 2 == o["restarts"]
    assert r["nconv"] < k
    assert r["nconv_ref_rule"] == o["nconv"] == k
    assert r["napplies"] == o["napplies"]
    # both return the Ritz values of the last restart; unconverged, they depend on the (different) random start blocks, so they are
    # compared through what holds for any start: descending, below the eigenvalues they approximate (Cauchy interlacing), and
    # of a 50-dimensional Krylov space's quality
    for ev in (r["evals"].astype(np.float64), o["evals"].astype(np.float64)):
        assert np.all(np.diff(ev) <= 1e-6) and np.all(ev <= evs[:k] + 1e-5)
        assert np.max(evs[:k] - ev) <= 0.25  # two restarts on a spectrum with gaps of 1 / n: far from converged, as intended
    U = r["U"].astype(np.float64)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 5e-5
    assert np.abs(np.sum(U * (A @ U), axis=0) - r["evals"]).max() <= 1e-4  # the values ARE the Rayleigh quotients of the returned vectors
    from isle_amd import IsleHipError
    with pytest.raises(IsleHipError, match="restarts exhausted"):
        hp.block_ks_dense(A32, k, maxit=2, tol=1e-7)
    # enough restarts: converges, both counts equal nev
    r3 = hp.block_ks_dense(seed_matrix(300, 1, 2)[0].astype(np.float32), k)
    assert r3["rc"] == 0 and r3["nconv"] == k == r3["nconv_ref_rule"]


@pytest.mark.parametrize("k,blk", [(15, 10), (25, 10), (37, 8)])
def test_ragged_nev_and_ncv(hp, k, blk):
    """nev / ncv that are not multiples of the block size (the CLI's ncv = 2k + 10 with k = 15, 25, ...): the reference
    overruns its basis; here the decomposition grows by whole blocks to at least ncv rows."""
    n = 400
    A, evs = seed_matrix(n, 2, k)
    r = hp.block_ks_dense(A.astype(np.float32), k, blk=blk, ncv=2 * k + 10, allow_noconv=True)
    assert np.max(np.abs(r["evals"] - evs[:k]) / evs[:k]) <= 2e-4
    U = r["U"].astype(np.float64)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 5e-5


def test_sparse_entry_accepts_ragged_topic_counts(hp, tiny20):
    """isle_hip_block_ks with num_topics = 15 (ncv = 40, blk = 10) against the dense truth."""
    import scipy.sparse as sp
    from conftest import upload
    B = tiny20
    upload(hp, B)
    r = hp.compute_block_ks(15, allow_noconv=True)
    S = sp.csc_matrix((B["vals"].astype(np.float64), B["rows"], B["offs"]), shape=(B["V"], B["D"]))
    lam = np.linalg.eigvalsh((S @ S.T).toarray())[::-1][:15]
    assert np.max(np.abs(np.sqrt(r["evals"]) - np.sqrt(lam)) / np.sqrt(lam)) <= 1e-4
