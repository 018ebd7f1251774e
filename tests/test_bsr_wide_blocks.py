"""Block sizes 5..8: the BSR kernels and blkdiag_vmul (csrc/hip/block.hip)
against scipy/numpy in fp64, then block_value and as_block solves end to
end."""
import numpy as np
import pytest
import scipy.sparse as sp

import amgcl_amd as am
from amgcl_amd.matrix import CSR

TOL = dict(rtol=1e-12, atol=1e-12)


@pytest.fixture(scope="module")
def hip():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from amgcl_amd.backend import make_backend

    return make_backend("hip")


def rand_bsr(rng, counts, B):
    """Square BSR with counts[i] dense random blocks in block row i."""
    nb = len(counts)
    indptr = np.concatenate([[0], np.cumsum(counts)])
    indices = np.concatenate(
        [np.sort(rng.choice(nb, k, replace=False)) for k in counts])
    data = rng.standard_normal((indptr[-1], B, B))
    return sp.bsr_matrix((data, indices, indptr), shape=(nb * B, nb * B))


def on_device(hip, A, B):
    from amgcl_amd.backend.hip import DeviceBSR

    Ad = DeviceBSR(CSR.from_scipy(A.tocsr()), B, hip.device)
    assert Ad.val.numel() == A.data.size  # same blocks, none merged or lost
    return Ad


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 6, 7, 8])
def test_wide_block_kernels(hip, B):
    rng = np.random.default_rng(B)
    # 203 block rows (no multiple of 4; 203 B is no multiple of 64 or 256):
    # empty rows, also eight in a row, odd and even counts, rows of 1, 2, 3
    # and about 30 blocks next to each other in one wave, an empty last row
    counts = rng.choice([0, 1, 2, 3, 29, 30], 203)
    counts[:6] = [0, 1, 2, 3, 29, 30]
    counts[8:16] = 0
    counts[-2:] = [3, 0]
    A = rand_bsr(rng, counts, B)
    n = A.shape[0]
    x, y0, rhs, m = rng.standard_normal((4, n))
    Ad = on_device(hip, A, B)
    xd, rd, md = hip.from_host(x), hip.from_host(rhs), hip.from_host(m)
    Ax = A @ x

    yd = hip.from_host(y0)  # beta = 0 must overwrite, not read, y
    hip.spmv(1.0, Ad, xd, 0.0, yd)
    np.testing.assert_allclose(hip.to_host(yd), Ax, **TOL)
    yd = hip.from_host(y0)
    hip.spmv(0.7, Ad, xd, -1.3, yd)
    np.testing.assert_allclose(hip.to_host(yd), 0.7 * Ax - 1.3 * y0, **TOL)
    out = hip.vector(n)
    hip.residual(rd, Ad, xd, out)
    np.testing.assert_allclose(hip.to_host(out), rhs - Ax, **TOL)
    # fused relax: t = M o (rhs - A x), then x += t
    hip.relax_diag(Ad, md, rd, xd, out)
    np.testing.assert_allclose(hip.to_host(out), m * (rhs - Ax), **TOL)
    np.testing.assert_allclose(hip.to_host(xd), x + m * (rhs - Ax), **TOL)

    nb = 1003
    M = rng.standard_normal((nb, B, B))
    v = rng.standard_normal(nb * B)
    wd = hip.vector(nb * B)
    hip.blkdiag_vmul(B, hip.from_host(M.ravel()), hip.from_host(v), wd)
    np.testing.assert_allclose(
        hip.to_host(wd), np.einsum("bij,bj->bi", M, v.reshape(nb, B)).ravel(), **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 8])
def test_wide_block_kernels_past_one_grid_pass(hip, B):
    """The launch is capped at 4096 blocks of 256 lanes, cut to a multiple of
    B blocks: 4095 * 256 / 5 = 209664 block rows per pass at B=5, 131072 at
    B=8.  Each size here is one full pass and a second of 4099 block rows.  A
    block row visited twice would apply beta twice."""
    rng = np.random.default_rng(100 + B)
    nb = {5: 209664, 8: 131072}[B] + 4099
    # 1..3 blocks a row (86 MB of values at B=5, 138 MB at B=8, the
    # least that 2^20 scalar rows a pass allow): the first
    # counts[i] of three distinct, sorted block columns near the diagonal
    counts = rng.integers(1, 4, nb)
    cols = np.sort((np.arange(nb)[:, None] + [0, 7, 19]) % nb, axis=1)
    indices = cols[np.arange(3) < counts[:, None]]
    indptr = np.concatenate([[0], np.cumsum(counts)])
    A = sp.bsr_matrix((rng.standard_normal((indices.size, B, B)), indices, indptr),
                      shape=(nb * B, nb * B))
    n = A.shape[0]
    x, y0 = rng.standard_normal((2, n))
    Ad = on_device(hip, A, B)
    xd, yd = hip.from_host(x), hip.from_host(y0)
    Ax = A @ x
    hip.spmv(0.7, Ad, xd, -1.3, yd)
    np.testing.assert_allclose(hip.to_host(yd), 0.7 * Ax - 1.3 * y0, **TOL)
    out = hip.vector(n)
    hip.residual(hip.from_host(y0), Ad, xd, out)
    np.testing.assert_allclose(hip.to_host(out), y0 - Ax, **TOL)


def kron_case(B):
    A0, _ = am.poisson3d(10)
    C = np.full((B, B), 0.15) + 0.85 * np.eye(B)
    A = CSR.from_scipy(sp.kron(A0.to_scipy(), sp.csr_matrix(C), format="csr"))
    return A, np.random.default_rng(3).standard_normal(A.nrows)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [6, 8])
def test_block_value_solve(hip, B):
    from amgcl_amd.backend.hip import DeviceBSR

    A, b = kron_case(B)
    iters = {}
    for bv in (B, 0):
        # Chebyshev, the smoother of the other block_value tests: at these
        # block sizes the off-diagonal 0.15 (B-1) of C reaches the diagonal 1,
        # which a pointwise diagonal smoother does not survive.  Levels here:
        # 1000 B rows as BSR, then two scalar ones no multiple of B.
        prm = {"precond": {"class": "amg", "coarse_enough": 300, "block_value": bv,
                           "relax": {"type": "chebyshev"}},
               "solver": {"type": "cg", "tol": 1e-8, "maxiter": 100}}
        s = am.make_solver(A, prm, backend=hip)
        x, iters[bv], _ = s(b)
        if bv:
            assert s._native is not None
            assert isinstance(s.P.levels[0].A, DeviceBSR)
            assert np.linalg.norm(b - A @ hip.to_host(x)) / np.linalg.norm(b) < 1e-7
    assert abs(iters[B] - iters[0]) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("B", [6, 8])
def test_as_block_solve(hip, B):
    A, b = kron_case(B)
    # coarse_enough 500 stops at two levels: the second (398 or 483 rows) is
    # no multiple of B, so it must be the directly solved one
    prm = {"precond": {"class": "amg", "coarse_enough": 500,
                       "relax": {"type": "as_block", "block_size": B,
                                 "base": {"type": "spai0"}}},
           "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}}
    _, it_cpu, _ = am.make_solver(A, prm)(b)
    x, it_hip, _ = am.make_solver(A, prm, backend=hip)(b)
    assert np.linalg.norm(b - A @ hip.to_host(x)) / np.linalg.norm(b) < 1e-7
    assert abs(it_hip - it_cpu) <= 2


def test_block_value_above_8_rejected():
    A, _ = am.poisson3d(6)
    with pytest.raises(ValueError, match="block_value"):
        am.make_solver(A, {"precond": {"class": "amg", "block_value": 9}})
