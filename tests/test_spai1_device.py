"""SPAI-1 on the device: the GPU setup kernel (amg_setup_spai1) against a
dense least-squares oracle, and SPAI-1 smoothing inside the native driver
against the generic per-kernel path.

Oracle (amgcl/relaxation/spai1.hpp:82-120, the row form): with I the pattern
of row i and D = A.toarray(), row i of M is lstsq(D[I, :].T, e_i).

Tolerance rtol = atol = 1e-12, the project's device-kernel tolerance.  A numpy
normal-equations + Cholesky twin of the kernel stays at 1.4e-15 max abs error
against the oracle on the matrix of test_tier_boundary_and_long_rows (worst
cond(G) 4.9e2), three orders inside that bound.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import amgcl_amd as am

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from amgcl_amd.backend import make_backend

    return make_backend("hip")


def oracle(a):
    """Row-form SPAI-1 values of the scipy CSR matrix a, in a's entry order."""
    D = a.toarray()
    out = np.empty(a.nnz)
    for i in range(a.shape[0]):
        b, e = a.indptr[i], a.indptr[i + 1]
        if e == b:
            continue
        ei = np.zeros(a.shape[1])
        ei[i] = 1.0
        out[b:e] = np.linalg.lstsq(D[a.indices[b:e], :].T, ei, rcond=None)[0]
    return out


def device_spai1(hip, a):
    from amgcl_amd.backend import hip_setup
    from amgcl_amd.backend.hip import DeviceCSR
    from amgcl_amd.matrix import CSR

    Ad = DeviceCSR(CSR.from_scipy(a), hip.device)
    M = hip_setup.spai1(Ad)
    # M has A's pattern and shares it, values are its own
    assert M.ptr is Ad.ptr and M.col is Ad.col
    assert (M.nrows, M.ncols) == a.shape
    return M.val.cpu().numpy()


def check(got, want, what):
    err = np.abs(got - want)
    print(f"{what}: max abs err {err.max():.3e}, "
          f"worst err/bound {(err / (TOL + TOL * np.abs(want))).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=TOL, atol=TOL)


def test_short_tier_symmetric(hip):
    """poisson3d(6): 216 rows, k <= 7, one wave per row.  The matrix is
    symmetric, so the host routine's column form coincides with the row form."""
    from amgcl_amd import _core

    A, _ = am.poisson3d(6)
    a = A.to_scipy().tocsr()
    a.sort_indices()
    assert np.diff(a.indptr).max() <= 7
    got = device_spai1(hip, a)
    check(got, oracle(a), "poisson3d(6) vs oracle")
    mp, mc, mv = _core.spai1(A.nrows, A.ptr, A.col, A.val)
    np.testing.assert_array_equal(np.asarray(mc), a.indices)
    check(got, np.asarray(mv), "poisson3d(6) vs _core.spai1")


def test_short_tier_single_entry_rows(hip):
    """k = 1: m = a_ii / a_ii^2, the SPAI-0 value."""
    d = np.array([2.0, -3.0, 0.5, 7.0, 1e3])
    a = sp.diags(d).tocsr()
    check(device_spai1(hip, a), 1.0 / d, "diagonal 5x5")


def boundary_matrix():
    n = 400
    S = sp.random(n, n, 0.02, random_state=5, format="lil")
    rng = np.random.RandomState(5)
    want = {10: 32, 11: 33, 12: 150}
    for r, k in want.items():
        S[r, :] = 0.0
        cols = rng.choice(np.delete(np.arange(n), r), k - 1, replace=False)
        S[r, cols] = rng.uniform(-1.0, 1.0, k - 1)
    S.setdiag(0.0)
    S = S.tocsr()
    S.eliminate_zeros()
    absS = abs(S)
    d = np.asarray(absS.sum(axis=1)).ravel() + np.asarray(absS.sum(axis=0)).ravel() + 1.0
    a = (S + sp.diags(d)).tocsr()
    a.sort_indices()
    lens = np.diff(a.indptr)
    for r, k in want.items():
        assert lens[r] == k, (r, lens[r])
    return a


def test_tier_boundary_and_long_rows(hip):
    """Nonsymmetric 400x400 with rows of exactly 32 (last of the short tier),
    33 (first of the long tier) and 150 entries.  Not compared with
    _core.spai1, which solves the column form and differs by design."""
    from amgcl_amd.backend._hiplib import lib

    assert lib().amg_spai1_short_max() == 32
    a = boundary_matrix()
    assert abs(a - a.T).max() > 0.1  # really nonsymmetric
    check(device_spai1(hip, a), oracle(a), "boundary matrix vs oracle")


def test_singular_row_raises(hip):
    """Rows 0 and 1 equal: G of either row's local system is [[2, 2], [2, 2]],
    whose second pivot (4.4e-16) is below k * eps * G[1][1] = 8.8e-16."""
    D = np.eye(8)
    D[0, :2] = 1.0
    D[1, :2] = 1.0
    with pytest.raises(RuntimeError, match="spai1: singular local system at row"):
        device_spai1(hip, sp.csr_matrix(D))


def spai1_prm(solver="cg", **precond):
    p = {"class": "amg", "coarse_enough": 300, "relax": {"type": "spai1"}}
    p.update(precond)
    return {"precond": p, "solver": {"type": solver, "tol": 1e-8, "maxiter": 100}}


def native_vs_generic(hip, s, A, b):
    """The parity criterion of test_native_driver_ilu0_jacobi (an in-place
    smoother whose native and generic forms round differently)."""
    assert s._native is not None, "native driver should engage for spai1"
    x1, it1, r1 = s(b)
    x1 = hip.to_host(x1).copy()
    native = s._native
    s._native = None  # generic path on the same hierarchy
    try:
        x2, it2, r2 = s(b)
    finally:
        s._native = native
    x2 = hip.to_host(x2)
    print(f"native {it1} its res {r1:.2e}; generic {it2} its res {r2:.2e}")
    assert r1 < 1e-8 and r2 < 1e-8
    assert abs(it1 - it2) <= 1, (it1, it2)
    assert np.linalg.norm(x1 - x2) / np.linalg.norm(x1) < 1e-8
    assert np.linalg.norm(b - A @ x1) / np.linalg.norm(b) < 1e-7


@pytest.fixture
def device_level0(hip, monkeypatch):
    """poisson3d(16) uploaded as a DeviceCSR, with every hip_setup.download
    recorded: the 4096-row level must never come back to the host."""
    from amgcl_amd.backend import hip_setup
    from amgcl_amd.backend.hip import DeviceCSR

    monkeypatch.setenv("AMGCL_HOST_HANDOFF", "500")
    downloads = []
    real = hip_setup.download

    def recording(M):
        downloads.append(M.nrows)
        return real(M)

    monkeypatch.setattr(hip_setup, "download", recording)
    A, b = am.poisson3d(16, rhs="random")
    return A, b, DeviceCSR(A, hip.device), downloads


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_device_built_no_download_native_parity(hip, device_level0, solver):
    A, b, Ad, downloads = device_level0
    s = am.make_solver(Ad, spai1_prm(solver), backend=hip)
    assert 4096 not in downloads, downloads
    native_vs_generic(hip, s, A, b)
    assert 4096 not in downloads, downloads


@pytest.mark.parametrize("precond", [
    {"npre": 2, "npost": 2, "ncycle": 2},
    {"direct_coarse": False},  # SPAI-1 on the coarsest level: zero-guess form
    {"pre_cycles": 2},
], ids=["w_cycle_2_2", "smooth_coarsest", "pre_cycles_2"])
def test_cycle_shapes(hip, device_level0, precond):
    A, b, Ad, downloads = device_level0
    s = am.make_solver(Ad, spai1_prm(**precond), backend=hip)
    assert 4096 not in downloads, downloads
    native_vs_generic(hip, s, A, b)


def test_host_built_hierarchy_native(hip):
    """Host CSR input: _core.spai1 + upload feeds the driver's descriptor."""
    A, b = am.poisson3d(16, rhs="random")
    s = am.make_solver(A, spai1_prm(), backend=hip)
    native_vs_generic(hip, s, A, b)


def test_precond_apply(hip):
    A, b = am.poisson3d(16, rhs="random")
    s = am.make_solver(A, spai1_prm(), backend=hip)
    assert s._native is not None
    rhs = hip.from_host(b)
    x = hip.vector(A.nrows)
    s._native.precond_apply(rhs, x)
    r = hip.vector(A.nrows)
    hip.residual(rhs, s.P.levels[0].A, x, r)
    assert float(r.norm()) < 0.5 * float(rhs.norm())  # one V-cycle contracts
    xg = hip.vector(A.nrows)
    s.P.apply(rhs, xg)
    rel = float((x - xg).norm()) / float(xg.norm())
    print(f"native vs generic V-cycle: rel diff {rel:.3e}")
    assert rel < 1e-10


def test_layout_has_spai1():
    from amgcl_amd.backend import native

    labels = [label for label, _ in native.desc_layout()]
    assert "offsetof(LevelDesc, spai1)" in labels
    assert labels[-1] == "offsetof(LevelDesc, ilu_b)"
    native._bind()
