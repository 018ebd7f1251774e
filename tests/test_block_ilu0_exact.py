"""block_ilu0 with solve="exact": the level-scheduled cooperative block
triangular solve (csrc/hip/block_sptrsv.hip) against the serial host sweeps
(_core.block_ilu0_solve), for every block size 1..8.

Kernel test matrix: S = kron(poisson3d(12), C) with C = I + 0.1 R R^T / B a
dense SPD BxB block, so S is SPD, every stored block is dense, and the block
pattern is the 7-point stencil on 12^3 points: 34 dependency levels per
factor, the widest holding 108 block rows; 13,824 scalar rows at B=8.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import amgcl_amd as am
from amgcl_amd import _core
from amgcl_amd.backend import make_backend
from amgcl_amd.matrix import CSR
from amgcl_amd.relaxation.block_ilu0 import BlockILU0

BLOCK_SIZES = list(range(1, 9))


@pytest.fixture(scope="module")
def hip():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_backend("hip")


@functools.lru_cache(maxsize=None)
def kron_case(B):
    """(S, host smoother, rhs, host solution); computed once, read-only."""
    A, _ = am.poisson3d(12)
    rng = np.random.default_rng(100 + B)
    R = rng.standard_normal((B, B))
    C = np.eye(B) + 0.1 * R @ R.T / B
    S = sp.kron(A.to_scipy(), C).tocsr()
    S.sort_indices()
    S = CSR(S.shape[0], S.shape[1], S.indptr, S.indices, S.data)
    host = BlockILU0(S, {"block_size": B}, make_backend("cpu"))
    z = rng.standard_normal(S.nrows)
    x = z.copy()
    _core.block_ilu0_solve(host.nb, B, host.bptr, host.bcol, host.lu,
                           host.dia, x)
    for a in (z, x):
        a.setflags(write=False)
    return S, host, z, x


def host_levels(host):
    dia32 = np.ascontiguousarray(host.dia, dtype=np.int32)
    return [np.asarray(_core.tri_levels(host.nb, host.bptr, host.bcol, dia32,
                                        lower)[0]) for lower in (True, False)]


# ---------------------------------------------------------------- no GPU ---

def test_solve_parameter_cpu():
    """solve=jacobi|exact is accepted; on the CPU backend both are the serial
    sweeps, so the results are bitwise equal; anything else is rejected."""
    cpu = make_backend("cpu")
    A, b, _ = am.generators.elasticity3d(4)
    assert BlockILU0.defaults()["solve"] == "jacobi"
    r_ex = BlockILU0(A, {"block_size": 3, "solve": "exact"}, cpu)
    r_ja = BlockILU0(A, {"block_size": 3, "solve": "jacobi"}, cpu)
    x_ex, x_ja = np.zeros(A.nrows), np.zeros(A.nrows)
    r_ex.apply(A, b, x_ex)
    r_ja.apply(A, b, x_ja)
    assert np.all(np.isfinite(x_ex)) and np.any(x_ex != 0.0)
    assert np.array_equal(x_ex, x_ja)
    with pytest.raises(ValueError, match="jacobi|exact"):
        BlockILU0(A, {"block_size": 3, "solve": "bogus"}, cpu)


@pytest.mark.parametrize("B", BLOCK_SIZES)
def test_kron_case_shape(B):
    """The premises the GPU tests rest on: a finite host solution, 34 levels
    per factor, 108 block rows in the widest."""
    S, host, z, x = kron_case(B)
    assert S.nrows == 12 ** 3 * B
    assert np.all(np.isfinite(x)) and np.abs(x).max() < 1.0
    for lp in host_levels(host):
        assert len(lp) - 1 == 34
        assert int(np.diff(lp).max()) == 108


def test_kron_case_b1_is_scalar_ilu0():
    S, host, z, x = kron_case(1)
    lu, dia = _core.ilu0_factor(S.nrows, S.ptr, S.col, S.val)
    y = z.copy()
    _core.ilu0_solve(S.nrows, S.ptr, S.col, np.asarray(lu), np.asarray(dia), y)
    np.testing.assert_allclose(x, y, rtol=2e-16, atol=2e-16)


# ------------------------------------------------------------------- GPU ---

@functools.lru_cache(maxsize=None)
def gpu_smoother(B):
    S = kron_case(B)[0]
    return BlockILU0(S, {"block_size": B, "solve": "exact"},
                     make_backend("hip"))


@pytest.mark.gpu
@pytest.mark.parametrize("B", BLOCK_SIZES)
def test_kernel_matches_host_sweeps(hip, B):
    """Tolerance 1e-12 as for the scalar twin (test_ilu0_exact_gpu_sptrsv):
    both sides may contract to FMA. Two runs from the same input must agree
    bitwise — a missed dependency shows as run-to-run drift."""
    S, host, z, x = kron_case(B)
    r = gpu_smoother(B)
    assert not hasattr(r, "_t0")  # no Jacobi work vectors
    z1, z2 = hip.from_host(z.copy()), hip.from_host(z.copy())
    r._solve_exact(z1)
    r._solve_exact(z2)
    g1, g2 = hip.to_host(z1), hip.to_host(z2)
    print(f"B={B} max|gpu-host|={np.abs(g1 - x).max():.3e}")
    np.testing.assert_allclose(g1, x, rtol=1e-12, atol=1e-12)
    assert np.array_equal(g1, g2)


@pytest.mark.gpu
def test_b1_matches_scalar_exact(hip):
    from amgcl_amd.relaxation.ilu0 import ILU0

    A, _ = am.poisson3d(16)
    z = np.random.default_rng(5).standard_normal(A.nrows)
    zs, zb = hip.from_host(z.copy()), hip.from_host(z.copy())
    ILU0(A, {"solve": "exact"}, hip)._solve_exact(zs)
    BlockILU0(A, {"block_size": 1, "solve": "exact"}, hip)._solve_exact(zb)
    np.testing.assert_allclose(hip.to_host(zb), hip.to_host(zs),
                               rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 8])
def test_grid_stride_and_multiblock_sync(hip, B):
    """One workgroup striding over each level and the automatic grid run the
    same per-row arithmetic, so the results agree bitwise."""
    from amgcl_amd.backend._hiplib import check, lib
    from amgcl_amd.backend.hip import _stream

    S, host, z, x = kron_case(B)
    r = gpu_smoother(B)
    lp, lr, up, ur = r._lev

    grid, block, group = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for lower in (1, 0):
        check(lib().amg_bsr_sptrsv_geometry(
            B, lower, ctypes.byref(grid), ctypes.byref(block),
            ctypes.byref(group)), "geometry")
        print(f"B={B} lower={lower} grid={grid.value} block={block.value} "
              f"group={group.value}")
        assert 1 <= grid.value <= 2048
    # the widest level exceeds one pass of one workgroup: max_blocks=1 strides
    for levptr in (lp, up):
        widest = int(np.diff(levptr.cpu().numpy()).max())
        assert widest > block.value // group.value

    def run(max_blocks):
        zd = hip.from_host(z.copy())
        check(lib().amg_bsr_sptrsv_f64(
            r._nlev[0], lp.data_ptr(), lr.data_ptr(), B, r.L.ptr.data_ptr(),
            r.L.col.data_ptr(), r.L.val.data_ptr(), 0, zd.data_ptr(), 1,
            max_blocks, _stream()), "lower")
        check(lib().amg_bsr_sptrsv_f64(
            r._nlev[1], up.data_ptr(), ur.data_ptr(), B, r.U.ptr.data_ptr(),
            r.U.col.data_ptr(), r.U.val.data_ptr(), r.Dinv.data_ptr(),
            zd.data_ptr(), 0, max_blocks, _stream()), "upper")
        return hip.to_host(zd)

    one, auto = run(1), run(0)
    np.testing.assert_allclose(auto, x, rtol=1e-12, atol=1e-12)
    assert np.array_equal(one, auto)


@pytest.mark.gpu
def test_bad_block_size_is_invalid_value(hip):
    from amgcl_amd.backend._hiplib import lib

    for bsize in (0, 9):
        assert lib().amg_bsr_sptrsv_f64(0, 0, 0, bsize, 0, 0, 0, 0, 0, 1, 0,
                                        0) == 1  # hipErrorInvalidValue


def _solve(A, b, relax, backend):
    prm = {"precond": {"class": "amg", "coarse_enough": 500, "relax": relax},
           "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}}
    if backend == "hip":
        # BSR level storage: a GPU storage format, the same operator
        prm["precond"]["block_value"] = 3
    s = am.make_solver(A, prm, backend=backend)
    x, iters, resid = s(b)
    xh = x if isinstance(x, np.ndarray) else s.backend.to_host(x)
    true = np.linalg.norm(b - A.to_scipy() @ xh) / np.linalg.norm(b)
    return iters, resid, true


@pytest.mark.gpu
def test_end_to_end_amg(hip):
    """AMG + CG on elasticity: the GPU's exact sweeps reproduce the CPU
    twin's iteration count to within 1 (summation order; the allowance
    test_hip_kernels.py uses for CSR vs SELL) and are no weaker than the
    iterated-Jacobi apply."""
    A, b, _ = am.generators.elasticity3d(8)
    exact = {"type": "block_ilu0", "block_size": 3, "solve": "exact"}
    it_gpu, resid, true = _solve(A, b, exact, "hip")
    assert resid < 1e-8
    assert true < 1e-7
    it_cpu, r_cpu, _ = _solve(A, b, exact, "cpu")
    assert r_cpu < 1e-8
    it_jac, r_jac, _ = _solve(
        A, b, {"type": "block_ilu0", "block_size": 3, "solve": "jacobi"},
        "hip")
    assert r_jac < 1e-8
    print(f"iterations: gpu exact {it_gpu}, cpu {it_cpu}, gpu jacobi {it_jac}")
    assert abs(it_gpu - it_cpu) <= 1, (it_gpu, it_cpu)
    assert it_gpu <= it_jac + 1, (it_gpu, it_jac)


@pytest.mark.gpu
def test_block_size_6_single_level(hip):
    """block_size 6 has no BSR SpMV kernel, so only the exact path can apply
    it on the GPU. 648 rows = 108 block rows."""
    A, b, _ = am.generators.elasticity3d(6)
    assert A.nrows == 648

    def solve(backend):
        s = am.make_solver(
            A, {"precond": {"class": "relaxation", "type": "block_ilu0",
                            "block_size": 6, "solve": "exact"},
                "solver": {"type": "cg", "tol": 1e-8, "maxiter": 200}},
            backend=backend)
        x, iters, resid = s(b)
        assert resid < 1e-8
        return iters

    it_gpu, it_cpu = solve("hip"), solve("cpu")
    print(f"iterations: gpu {it_gpu}, cpu {it_cpu}")
    assert abs(it_gpu - it_cpu) <= 1, (it_gpu, it_cpu)
