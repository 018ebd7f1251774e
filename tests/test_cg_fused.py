"""Vector kernels folded into SELL passes (sell_k modes 3 to 5) and the CG
driver that uses them, against the unfused kernel sequence of the same build.

Kernel level: each fused mode against the kernels it replaces, through the C
entry points, on the padded and the compact image of two matrices.  Driver
level: make_solver with the fused paths on (default) and off (AMGCL_NO_FUSE=1,
read at driver creation).
"""
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import amgcl_amd as am
from amgcl_amd.backend import _hiplib

NP_DTYPE = {"f64": np.float64, "f32": np.float32}
BITS = {"f64": np.int64, "f32": np.int32}
U53 = 2.0 ** -53
BETA = 0.3
GARBAGE = 1e300  # what `out` holds before a fused dot is launched


# ---------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------
def _csr(name, rng):
    """'ragged': 67 rows (one full slice plus a 3-row tail) by 80 columns;
    rows 13 and 66 (the last) are empty, row 40 has 70 entries, the others 1
    to 9.  'wrap': 64 * 5 + 1 square; row 70 is empty, row 200 has 9 entries
    (more than SELLC_U = 4 slots, so the slot chunk wraps), the others 1 to
    4."""
    if name == "ragged":
        n, ncols = 67, 80
        lens = rng.integers(1, 10, size=n)
        lens[[13, 66]] = 0
        lens[40] = 70
    else:
        n = ncols = 64 * 5 + 1
        lens = rng.integers(1, 5, size=n)
        lens[70] = 0
        lens[200] = 9
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=ptr[1:])
    col = np.concatenate([np.sort(rng.choice(ncols, size=k, replace=False))
                          for k in lens]).astype(np.int32)
    return ncols, ptr, col


@pytest.fixture(scope="module")
def cases(hip_backend):
    """(matrix, dtype, image) -> the SELL image and device vectors, built once
    and never written.  M, rhs, s, p and x have one entry per column, since
    the fused modes gather from them."""
    import torch

    from amgcl_amd.backend.hip import DeviceCSR

    out = {}
    for mi, mname in enumerate(("ragged", "wrap")):
        for di, dt in enumerate(NP_DTYPE):
            rng = np.random.default_rng(300 + 10 * mi + di)
            ncols, ptr, col = _csr(mname, rng)
            n = len(ptr) - 1
            rnd = lambda m: rng.standard_normal(m).astype(NP_DTYPE[dt])
            host = dict(ptr=ptr, col=col, val=rnd(len(col)), M=rnd(ncols), rhs=rnd(ncols),
                        s=rnd(ncols), p=rnd(ncols), x=rnd(ncols))
            dev = {k: torch.from_numpy(v).to(hip_backend.device) for k, v in host.items()}
            for image in ("padded", "compact"):
                S = DeviceCSR.from_tensors(n, ncols, dev["ptr"], dev["col"], dev["val"])
                S = S.build_sell(compact=(image == "compact"))
                assert (S.smask is not None) == (image == "compact")
                assert S.nslice == (n + 63) // 64
                out[mname, dt, image] = types.SimpleNamespace(
                    n=n, ncols=ncols, dt=dt, S=S, dev=dev, torch=torch,
                    device=hip_backend.device)
    return out


def _stream():
    from amgcl_amd.backend.hip import _stream as s

    return s()


def _fused_image(S):
    """Leading arguments of the fused entry points (either image)."""
    if S.smask is not None:
        return (S.nrows, S.nslice, S.moff.data_ptr(), S.scol.data_ptr(), S.sval.data_ptr(),
                0, S.smask.data_ptr(), S.ptr.data_ptr())
    return (S.nrows, S.nslice, S.soff.data_ptr(), S.scol.data_ptr(), S.sval.data_ptr(),
            S.srows.data_ptr() if S.srows is not None else 0, 0, 0)


def _call(name, *args):
    _hiplib.check(getattr(_hiplib.lib(), name)(*args, _stream()), name)


def _nan(c, m):
    return c.torch.full((m,), float("nan"), dtype=c.dev["val"].dtype, device=c.device)


def _same_bits(got, want, dt, what):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.shape == want.shape, what
    differ = int((got.view(BITS[dt]) != want.view(BITS[dt])).sum())
    print(f"{what}: {differ} of {got.size} entries differ in bits")
    assert differ == 0, what


def _check_dot(out, a, b, what):
    """|out - a·b| <= n 2^-53 sum|a_i b_i|: the worst-case bound of a length-n
    fp64 dot product summed in any order, against the exact value."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    exact = sum(Fraction(float(u)) * Fraction(float(v)) for u, v in zip(a, b))
    bound = len(a) * U53 * float(np.abs(a * b).sum())
    err = abs(float(Fraction(float(out.cpu().numpy()[0])) - exact))
    print(f"{what}: dot error {err:.3e}, bound {bound:.3e}")
    assert math.isfinite(err) and err <= bound, what


@pytest.mark.gpu
@pytest.mark.parametrize("image", ["padded", "compact"])
@pytest.mark.parametrize("dt", list(NP_DTYPE))
@pytest.mark.parametrize("mname", ["ragged", "wrap"])
def test_zero_guess_residual(cases, mname, dt, image):
    """Mode 3: u and t bit for bit those of relax_zero followed by the mode-1
    residual of the same image."""
    c = cases[mname, dt, image]
    d, S = c.dev, c.S
    u_ref, t_ref = _nan(c, c.ncols), _nan(c, c.n)
    _call("amg_relax_zero_" + dt, c.ncols, d["M"].data_ptr(), d["rhs"].data_ptr(),
          u_ref.data_ptr())
    _call(f"amg_{S.sell_name}_residual_{dt}", *S.sell_args, d["rhs"].data_ptr(),
          u_ref.data_ptr(), t_ref.data_ptr())
    u, t = _nan(c, c.n), _nan(c, c.n)
    _call("amg_sell_zero_residual_" + dt, *_fused_image(S), d["M"].data_ptr(),
          d["rhs"].data_ptr(), u.data_ptr(), t.data_ptr())
    _same_bits(u, u_ref[:c.n], dt, f"mode 3 u {mname} {dt} {image}")
    _same_bits(t, t_ref, dt, f"mode 3 t {mname} {dt} {image}")
    assert bool(c.torch.isfinite(t).all())


@pytest.mark.gpu
@pytest.mark.parametrize("image", ["padded", "compact"])
@pytest.mark.parametrize("mname", ["ragged", "wrap"])
def test_relax_dot(cases, mname, image):
    """Mode 4: xn bit for bit that of mode 2, out = rhs · xn within the bound
    of _check_dot; out holds garbage before the call."""
    c = cases[mname, "f64", image]
    d, S = c.dev, c.S
    xn_ref, xn = _nan(c, c.n), _nan(c, c.n)
    _call(f"amg_{S.sell_name}_relax_f64", *S.sell_args, d["M"].data_ptr(),
          d["rhs"].data_ptr(), d["x"].data_ptr(), xn_ref.data_ptr())
    out = c.torch.full((1,), GARBAGE, dtype=c.torch.float64, device=c.device)
    _call("amg_sell_relax_dot_f64", *_fused_image(S), d["M"].data_ptr(),
          d["rhs"].data_ptr(), d["x"].data_ptr(), xn.data_ptr(), out.data_ptr())
    _same_bits(xn, xn_ref, "f64", f"mode 4 xn {mname} {image}")
    _check_dot(out, d["rhs"][:c.n], xn, f"mode 4 {mname} {image}")


@pytest.mark.gpu
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("image", ["padded", "compact"])
@pytest.mark.parametrize("mname", ["ragged", "wrap"])
def test_pupdate_spmv_dot(cases, mname, image, first):
    """Mode 5: p_new bit for bit axpby(1, s, beta, p), q bit for bit the
    mode-0 spmv of that stored p_new, out = q · p_new within the bound.  With
    `first`, p is all NaN and must not be read: p_new = s, q = A s, finite."""
    c = cases[mname, "f64", image]
    d, S = c.dev, c.S
    if first:
        p, p_ref = _nan(c, c.ncols), d["s"].clone()
    else:
        p, p_ref = d["p"], d["p"].clone()
        _call("amg_axpby_f64", c.ncols, 1.0, d["s"].data_ptr(), BETA, p_ref.data_ptr())
    q_ref = _nan(c, c.n)
    _call(f"amg_{S.sell_name}_spmv_f64", *S.sell_args, p_ref.data_ptr(), 1.0, 0.0,
          q_ref.data_ptr())
    p_new, q = _nan(c, c.n), _nan(c, c.n)
    out = c.torch.full((1,), GARBAGE, dtype=c.torch.float64, device=c.device)
    _call("amg_sell_pupdate_spmv_dot_f64", *_fused_image(S), d["s"].data_ptr(),
          p.data_ptr(), BETA, int(first), p_new.data_ptr(), q.data_ptr(), out.data_ptr())
    what = f"mode 5 {mname} {image} first={first}"
    assert bool(c.torch.isfinite(p_new).all()) and bool(c.torch.isfinite(q).all()), what
    _same_bits(p_new, p_ref[:c.n], "f64", what + " p_new")
    _same_bits(q, q_ref, "f64", what + " q")
    _check_dot(out, q, p_new, what)


# ---------------------------------------------------------------------------
# driver level
# ---------------------------------------------------------------------------
TOL = 1e-8
CONFIGS = {
    "default": ({}, "cg"),
    "npre2": ({"npre": 2}, "cg"),
    "npost0": ({"npost": 0}, "cg"),
    "ncycle2": ({"ncycle": 2}, "cg"),
    "pre_cycles2": ({"pre_cycles": 2}, "cg"),
    "mixed": ({"precision": "mixed"}, "cg"),
    "block2": ({"block_value": 2}, "cg"),
    "chebyshev": ({"relax": {"type": "chebyshev"}}, "cg"),
    "bicgstab": ({}, "bicgstab"),
}
# Right-hand-side seeds.  Candidates were 0, 1 and 2 for every configuration;
# a seed is kept only if two unfused runs give the same iteration count on
# both right-hand sides.  All 27 did, so none is dropped (0 of 27, allowed 1
# in 5).
SEEDS = {name: (0, 1, 2) for name in CONFIGS}
# max|x_a - x_b| / max|x| allowed between the fused and the unfused side: 10 x
# the largest figure measured between two unfused runs (their dots are summed
# in atomic order already).  Measured over all seeds and both right-hand sides:
#   fp64 cycle (every configuration but mixed): unfused vs unfused <= 5.484e-16,
#       fused or ungraphed vs unfused <= 4.113e-16
#   mixed (fp32 cycle): unfused vs unfused <= 1.323e-14,
#       fused or ungraphed vs unfused <= 1.493e-14
X_BOUND = {name: 10 * 5.484e-16 for name in CONFIGS}
X_BOUND["mixed"] = 10 * 1.323e-14


@pytest.fixture(scope="module")
def poisson24():
    A, _ = am.poisson3d(24)
    return A


def solve_case(A, backend, name, seed, monkeypatch, fuse=True, graph=True):
    """Build the solver of configuration `name` with the fused paths on or
    off, solve for the seeded right-hand side and then, on the same solver,
    for a second one.  -> [(x, iters, resid, true relative residual)] * 2"""
    extra, solver = CONFIGS[name]
    for var, on in (("AMGCL_NO_FUSE", fuse), ("AMGCL_NO_GRAPH", graph)):
        if on:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, "1")
    precond = {"class": "amg", "coarse_enough": 300, "sell_min_rows": 64}
    precond.update(extra)
    s = am.make_solver(A, {"precond": precond,
                           "solver": {"type": solver, "tol": TOL, "maxiter": 100}},
                       backend=backend)
    assert s._native is not None, name
    if name not in ("block2",):
        assert sum(1 for l in s.P.levels if getattr(l.A, "nslice", 0)) >= 2, name
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        b = rng.standard_normal(A.nrows)
        x, it, res = s(b)
        x = backend.to_host(x)
        true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
        out.append((x, it, res, true))
    return out


def x_diff(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_driver_fused_vs_unfused(hip_backend, poisson24, monkeypatch, name):
    """Fused against unfused (AMGCL_NO_FUSE=1) on Poisson 24^3 with SELL
    images from 64 rows up: both reach the tolerance, the true relative
    residual (host, fp64) is <= tol, the iteration counts are equal and x
    agrees within X_BOUND; the same for a second right-hand side on the same
    solver, and for the fused side with AMGCL_NO_GRAPH=1 (graph cache key,
    pointer parity).

    Seeds: candidates 0, 1, 2 per configuration, kept where two unfused runs
    agree on the iteration count; 0 of 27 dropped.  x bound: 10 x the measured
    unfused-vs-unfused figure, 5.484e-16 for the fp64 cycle and 1.323e-14 for
    mixed; fused-vs-unfused measured 4.113e-16 and 1.493e-14 (SEEDS, X_BOUND
    above; profiles/README.md, "CG solve: fused SELL passes").
    """
    for seed in SEEDS[name]:
        unfused = solve_case(poisson24, hip_backend, name, seed, monkeypatch, fuse=False)
        fused = solve_case(poisson24, hip_backend, name, seed, monkeypatch)
        eager = solve_case(poisson24, hip_backend, name, seed, monkeypatch, graph=False)
        for k in range(2):
            for side, run in (("unfused", unfused), ("fused", fused), ("eager", eager)):
                x, it, res, true = run[k]
                print(f"{name} seed {seed} rhs {k} {side}: {it} it, res {res:.3e}, "
                      f"true {true:.3e}")
                assert res <= TOL and true <= TOL, (name, seed, k, side)
            assert fused[k][1] == unfused[k][1] == eager[k][1], (name, seed, k)
            for side, run in (("fused", fused), ("eager", eager)):
                dx = x_diff(run[k][0], unfused[k][0])
                print(f"{name} seed {seed} rhs {k} {side} vs unfused: dx {dx:.3e}")
                assert dx <= X_BOUND[name], (name, seed, k, side, dx)
