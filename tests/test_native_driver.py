"""Native C++ solve driver vs the generic Python orchestration."""
import numpy as np
import pytest

import amgcl_amd as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from amgcl_amd.backend import make_backend

    return make_backend("hip")


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_native_matches_python(hip, solver):
    A, b = am.poisson3d(40, rhs="random")
    prm = {"solver": {"type": solver, "tol": 1e-8, "maxiter": 100}}
    s = am.make_solver(A, prm, backend=hip)
    assert s._native is not None, "native driver should engage for this config"
    x1, it1, res1 = s(b)

    s._native = None  # force generic path on the same hierarchy
    x2, it2, res2 = s(b)
    assert res1 < 1e-8 and res2 < 1e-8
    assert it1 == it2
    r = b - A @ hip.to_host(x1)
    assert np.linalg.norm(r) / np.linalg.norm(b) < 1e-7


def test_native_w_cycle(hip):
    A, b = am.poisson3d(32, rhs="random")
    s = am.make_solver(
        A,
        {
            "precond": {"class": "amg", "ncycle": 2, "npre": 2, "npost": 2},
            "solver": {"type": "cg", "tol": 1e-8, "maxiter": 100},
        },
        backend=hip,
    )
    assert s._native is not None
    x, iters, resid = s(b)
    assert resid < 1e-8
    r = b - A @ hip.to_host(x)
    assert np.linalg.norm(r) / np.linalg.norm(b) < 1e-7


def test_native_rejects_unsupported(hip):
    # multicolor Gauss-Seidel is outside the driver's smoother set
    A, b = am.poisson3d(16)
    s = am.make_solver(
        A,
        {
            "precond": {"class": "amg", "relax": {"type": "gauss_seidel"}},
            "solver": {"type": "cg", "tol": 1e-8},
        },
        backend=hip,
    )
    assert s._native is None
    x, iters, resid = s(b)
    assert resid < 1e-8


def test_native_driver_ilu0_jacobi(hip):
    """ILU(0) with iterated-Jacobi triangular solves runs inside the native
    driver (ilu_solve.hpp semantics); the exact-sptrsv variant stays on the
    generic path (cooperative kernels are not graph-capturable)."""
    A, b = am.poisson3d(24, rhs="random", anisotropy=50.0)
    prm = {"precond": {"class": "amg", "coarse_enough": 300,
                       "relax": {"type": "ilu0"}},
           "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}}
    s = am.make_solver(A, prm, backend=hip)
    assert s._native is not None
    x1, it1, r1 = s(b)
    assert r1 < 1e-8

    import copy

    prm2 = copy.deepcopy(prm)
    prm2["solver"]["verbose"] = True
    s2 = am.make_solver(A, prm2, backend=hip)
    assert s2._native is None
    x2, it2, r2 = s2(b)
    assert abs(it1 - it2) <= 1, (it1, it2)
    xa, xb = hip.to_host(x1), hip.to_host(x2)
    assert np.linalg.norm(xa - xb) / np.linalg.norm(xa) < 1e-8

    prm3 = copy.deepcopy(prm)
    prm3["precond"]["relax"]["solve"] = "exact"
    s3 = am.make_solver(A, prm3, backend=hip)
    assert s3._native is None  # exact sptrsv -> generic path
    x3, it3, r3 = s3(b)
    assert r3 < 1e-8


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_native_mixed_precision(hip, solver):
    """fp32 hierarchy through the native driver (fp64 Krylov + cast-bracketed
    fp32 V-cycle) matches the generic mixed path exactly."""
    A, b = am.poisson3d(40, rhs="random")
    prm = {"precond": {"class": "amg", "precision": "mixed"},
           "solver": {"type": solver, "tol": 1e-8, "maxiter": 100}}
    s = am.make_solver(A, prm, backend=hip)
    assert s._native is not None and s._native._mixed
    x1, it1, res1 = s(b)
    s._native = None  # generic mixed path on the same hierarchy
    x2, it2, res2 = s(b)
    assert res1 < 1e-8 and res2 < 1e-8
    assert it1 == it2
    r = b - A @ hip.to_host(x1)
    assert np.linalg.norm(r) / np.linalg.norm(b) < 1e-7


def test_native_precond_apply(hip):
    """Standalone V-cycle application through amg_driver_precond — the inner
    op of the distributed block preconditioner."""
    A, b = am.poisson3d(24, rhs="random")
    s = am.make_solver(A, {"solver": {"type": "cg", "tol": 1e-8, "maxiter": 50}},
                       backend=hip)
    assert s._native is not None
    rhs = hip.from_host(b)
    x = hip.vector(A.nrows)
    s._native.precond_apply(rhs, x)
    r = hip.vector(A.nrows)
    hip.residual(rhs, s.P.levels[0].A, x, r)
    assert float(r.norm()) < 0.5 * float(rhs.norm())  # one V-cycle contracts


def test_local_block_precond_on_device(hip):
    """LocalBlockPrecond with a device-resident local block + native V-cycle
    apply — the per-rank path of the multi-GPU scale bench (single-rank gloo
    group; RCCL exchange is a no-op at world 1)."""
    import os

    import torch.distributed as dist

    from amgcl_amd.parallel.dist_backend import DistBackend
    from amgcl_amd.parallel.precond import LocalBlockPrecond

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29553")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    try:
        A, b = am.poisson3d(24, rhs="random")
        backend = DistBackend(hip)
        dist_A = backend.matrix(A)
        P = LocalBlockPrecond(dist_A, {"class": "amg", "coarse_enough": 300},
                              backend)
        assert P._native is not None  # the native driver must engage
        rhs = hip.from_host(b)
        x = hip.vector(A.nrows)
        P.apply(rhs, x)
        r = hip.vector(A.nrows)
        backend.residual(rhs, dist_A, x, r)
        assert float(r.norm()) < 0.5 * float(rhs.norm())
    finally:
        if created:
            dist.destroy_process_group()


def test_native_driver_chebyshev(hip):
    """The native driver now runs Chebyshev smoothing (driver twin of
    relaxation/chebyshev.py): engages for AMG+chebyshev+CG and matches the
    generic per-kernel path."""
    import amgcl_amd as am

    A, b = am.poisson3d(24, rhs="random")
    prm = {"precond": {"class": "amg", "coarse_enough": 300,
                       "relax": {"type": "chebyshev"}},
           "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}}
    s = am.make_solver(A, prm, backend=hip)
    assert s._native is not None, "chebyshev config should engage the driver"
    x1, it1, r1 = s(b)
    assert r1 < 1e-8

    import copy

    prm2 = copy.deepcopy(prm)
    prm2["solver"]["verbose"] = True  # verbose forces the generic path
    s2 = am.make_solver(A, prm2, backend=hip)
    assert s2._native is None
    x2, it2, r2 = s2(b)
    # the native CG fuses the x/r update (cg_tail), so the residual history
    # differs in the last bits — allow a 1-iteration difference
    assert abs(it1 - it2) <= 1, (it1, it2)
    assert r2 < 1e-8
    xa, xb = hip.to_host(x1), hip.to_host(x2)
    assert np.linalg.norm(xa - xb) / np.linalg.norm(xa) < 1e-8


def test_native_driver_bsr_levels(hip):
    """BSR (block_value) hierarchies run through the native driver
    (elasticity/BASELINE config #3 shape)."""
    import amgcl_amd as am
    from amgcl_amd.generators import elasticity3d, rigid_body_modes

    n = 12
    Ah, bh, coords = elasticity3d(n)
    B = rigid_body_modes(coords)
    bd = hip.from_host(bh)
    prm = {"precond": {"class": "amg", "block_value": 3,
                       "keep_host_matrices": True,
                       "relax": {"type": "chebyshev"},
                       "coarsening": {"type": "smoothed_aggregation",
                                      "nullspace_raw": B, "block_size": 3,
                                      "estimate_spectral_radius": True,
                                      "power_iters": 10}},
           "solver": {"type": "cg", "tol": 1e-6, "maxiter": 300}}
    s = am.make_solver(Ah, prm, backend=hip)
    assert s._native is not None, "BSR+chebyshev should engage the driver"
    x, iters, resid = s(bd)
    assert resid < 1e-6
    xh = hip.to_host(x)
    assert np.linalg.norm(bh - Ah @ xh) / np.linalg.norm(bh) < 1e-5


def _storage_case(storage, solver):
    """(A, b, prm, tol) for one fine-operator storage of the Krylov loop."""
    if storage == "bsr":
        from amgcl_amd.generators import elasticity3d, rigid_body_modes

        A, b, coords = elasticity3d(12)
        precond = {"class": "amg", "block_value": 3, "keep_host_matrices": True,
                   "relax": {"type": "chebyshev"},
                   "coarsening": {"type": "smoothed_aggregation",
                                  "nullspace_raw": rigid_body_modes(coords),
                                  "block_size": 3,
                                  "estimate_spectral_radius": True,
                                  "power_iters": 10}}
        tol, maxiter = 1e-6, 300
    else:
        A, b = am.poisson3d(24, rhs="random")
        precond = {"class": "amg", "coarse_enough": 300}
        if storage == "sell":
            precond.update({"sell": "auto", "sell_min_rows": 1,
                            "sell_min_mean": 0.0})
        elif storage == "sell_sigma":
            precond["sell"] = "off"  # the test builds the sigma-sorted images
        elif storage == "mixed":
            precond = {"class": "amg", "precision": "mixed"}
        tol, maxiter = 1e-8, 100
    prm = {"precond": precond,
           "solver": {"type": solver, "tol": tol, "maxiter": maxiter}}
    return A, b, prm, tol


def _sigma_sell_images(s):
    """Give A, P and R of every level a sigma-sorted SELL image (the sort's
    size and padding gates lowered so it engages at test size), then attach a
    fresh native driver that sees them."""
    from amgcl_amd.backend.native import try_native

    ops = [M for l in s.P.levels for M in (l.A, l.P, l.R) if M is not None]
    for M in ops:
        M.build_sell(sigma=128, sigma_min_rows=0, sigma_min_pad=0.0)
        assert M.nslice and M.srows is not None
    assert len(ops) == 3 * len(s.P.levels) - 2 and len(s.P.levels) >= 2
    s._native = try_native(s)


@pytest.mark.parametrize("storage", ["csr", "sell", "bsr", "mixed", "sell_sigma"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_native_storage_matrix(hip, solver, storage):
    """Both native Krylov loops against the generic path for every storage
    the fine operator can carry (CSR, SELL, BSR, fp64 override of a mixed
    hierarchy, SELL with sigma-sorted rows on A, P and R)."""
    from amgcl_amd.backend.hip import DeviceBSR

    A, b, prm, tol = _storage_case(storage, solver)
    s = am.make_solver(A, prm, backend=hip)
    if storage == "sell_sigma":
        _sigma_sell_images(s)
    assert s._native is not None, "native driver should engage for this config"
    A0 = s.P.levels[0].A
    assert isinstance(A0, DeviceBSR) == (storage == "bsr")
    assert bool(getattr(A0, "nslice", 0)) == (storage in ("sell", "sell_sigma"))
    assert s._native._mixed == (storage == "mixed")
    x1, it1, res1 = s(b)

    s._native = None  # generic path on the same hierarchy
    x2, it2, res2 = s(b)
    r = b - A @ hip.to_host(x1)
    true = np.linalg.norm(r) / np.linalg.norm(b)
    print(f"storage_matrix {solver}/{storage}: native {it1} it {res1:.3e}, "
          f"generic {it2} it {res2:.3e}, true {true:.3e}")
    if solver == "cg":
        # the native CG fuses the x/r update (cg_tail): last-bit differences
        assert abs(it1 - it2) <= 1, (it1, it2)
    else:
        assert it1 == it2
    assert res1 < tol and res2 < tol
    assert true < 10 * tol


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_native_zero_rhs(hip, solver):
    """b = 0 takes the driver's shortcut: x is cleared, nothing iterates."""
    import torch

    A, _ = am.poisson3d(16)
    s = am.make_solver(A, {"solver": {"type": solver, "tol": 1e-8, "maxiter": 100}},
                       backend=hip)
    assert s._native is not None
    x0 = hip.from_host(np.ones(A.nrows))
    x, iters, resid = s(np.zeros(A.nrows), x=x0)
    assert iters == 0 and resid == 0.0
    assert x is x0 and torch.count_nonzero(x).item() == 0


def test_leveldesc_layout():
    """The ctypes OpDescC / LevelDescC and the compiled structs agree on both
    sizes and on the offset of every OpDesc member and every top-level
    LevelDesc member (what _bind() enforces)."""
    import ctypes

    from amgcl_amd.backend import native

    L = native._bind()
    ours = native.desc_layout()
    assert [label for label, _ in ours[:2]] == ["sizeof(OpDesc)", "sizeof(LevelDesc)"]
    assert len(ours) == 2 + len(native.OpDescC._fields_) + len(native.LevelDescC._fields_)
    assert ours[0][1] == ctypes.sizeof(native.OpDescC)
    assert ours[1][1] == ctypes.sizeof(native.LevelDescC)
    assert ours[-1] == ("offsetof(LevelDesc, ilu_b)", native.LevelDescC.ilu_b.offset)
    theirs = native.lib_desc_layout(L)
    assert len(theirs) == len(ours)
    for (label, mine), lib_value in zip(ours, theirs):
        assert mine == lib_value, label


@pytest.mark.gpu
def test_block_ilu0_on_hip():
    """block_ilu0 smoothing on the HIP backend: BSR L/U iterated-Jacobi
    triangular solves (generic path; block twin of the scalar GPU ILU)."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import numpy as np

    from amgcl_amd.generators import elasticity3d

    A, b, coords = elasticity3d(8)
    prm = {"precond": {"class": "amg", "coarse_enough": 500,
                       "relax": {"type": "block_ilu0", "block_size": 3}},
           "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}}
    s = am.make_solver(A, prm, backend="hip")
    x, iters, resid = s(b)
    assert resid < 1e-8
    xh = s.backend.to_host(x)
    true = np.linalg.norm(b - A.to_scipy() @ xh) / np.linalg.norm(b)
    assert true < 1e-7
    s2 = am.make_solver(A, prm)  # CPU twin: exact sweeps vs iterated-Jacobi
    x2, it2, r2 = s2(b)
    assert iters <= it2 + 10, (iters, it2)

    # the full CoupCons3D-class configuration: BSR level storage AND the
    # block-valued ILU smoother together (generic path)
    prm3 = {"precond": {"class": "amg", "coarse_enough": 500,
                        "block_value": 3,
                        "relax": {"type": "block_ilu0", "block_size": 3}},
            "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}}
    s3 = am.make_solver(A, prm3, backend="hip")
    x3, it3, r3 = s3(b)
    assert r3 < 1e-8
    xh3 = s3.backend.to_host(x3)
    assert np.linalg.norm(b - A.to_scipy() @ xh3) / np.linalg.norm(b) < 1e-7
