"""Every arm of the host-side launch dispatch in csrc/hip/kernels.hip, on the
smallest inputs that can expose a wrong arm: each sub-wave width of the CSR
row kernels for each value type, each _f64/_f32 forwarder of the vector ops,
and the SELL launchers with and without a row permutation.  The exported
functions are called through lib() and compared with a float64/complex128
NumPy evaluation of the same arrays.

Tolerances are the ones the existing kernel tests use: rtol = atol = 1e-12
for fp64 (tests/test_hip_kernels.py; also used for complex128, whose kernels
do the same fp64 arithmetic and whose only existing bounds, the 1e-7/1e-8
solve residuals of tests/test_complex.py, are far looser), a maximum absolute
error of 1e-4 for fp32 results and 1e-3 for the fp32 dot
(test_f32_kernels_match_f64), and 1e-7 * sqrt(n) for the fp64 dot.
"""
import ctypes
import types

import numpy as np
import pytest

from amgcl_amd.backend import _hiplib

SUBWS = [0, 1, 2, 4, 8, 16, 32, 64]
NP_DTYPE = {"f64": np.float64, "f32": np.float32, "c128": np.complex128}

# _SIGS of the names whose entries are derived instead of listed, as they were
# listed by hand (I64 = c_int64, I32 = c_int, F64 = c_double, PTR = c_void_p);
# each _f32 twin had the signature of its _f64 entry
_CT = {"I64": ctypes.c_int64, "I32": ctypes.c_int, "F64": ctypes.c_double,
       "PTR": ctypes.c_void_p}
LISTED_SIGS = {
    "spmv": "I64 I64 PTR PTR PTR PTR F64 F64 PTR I32 PTR",
    "residual": "I64 I64 PTR PTR PTR PTR PTR PTR I32 PTR",
    "relax_diag": "I64 I64 PTR PTR PTR PTR PTR PTR PTR I32 PTR",
    "axpby": "I64 F64 PTR F64 PTR PTR",
    "axpbypcz": "I64 F64 PTR F64 PTR F64 PTR PTR",
    "vmul": "I64 F64 PTR PTR F64 PTR PTR",
    "fill": "I64 F64 PTR PTR",
    "dot": "I64 PTR PTR PTR PTR",
    "gather": "I64 PTR PTR PTR PTR",
    "scatter": "I64 PTR PTR PTR PTR",
    "gemv": "I64 PTR PTR PTR PTR",
    "sell_spmv": "I64 I64 PTR PTR PTR PTR PTR F64 F64 PTR PTR",
    "sell_residual": "I64 I64 PTR PTR PTR PTR PTR PTR PTR PTR",
    "sell_relax": "I64 I64 PTR PTR PTR PTR PTR PTR PTR PTR PTR",
    "sell_fill": "I64 I64 PTR PTR PTR PTR PTR PTR PTR PTR",
}


def test_sigs_table_and_symbols():
    """The derived _f32 entries equal the hand-listed table, and every name
    in _SIGS is exported by the built library (it cross-compiles, so this
    needs no GPU)."""
    for op, sig in LISTED_SIGS.items():
        want = [_CT[t] for t in sig.split()]
        for sfx in ("_f64", "_f32"):
            assert _hiplib._SIGS[f"amg_{op}{sfx}"] == want, op + sfx
    assert len(_hiplib._SIGS) == 72
    lib = _hiplib.lib()
    for name in _hiplib._SIGS:
        assert hasattr(lib, name), name


def test_unsupported_subw_is_invalid_value():
    """A sub-wave width the row kernels are not instantiated for is refused
    before anything is launched."""
    lib = _hiplib.lib()
    for sfx in ("_f64", "_f32"):
        assert getattr(lib, "amg_spmv" + sfx)(1, 1, 0, 0, 0, 0, 1.0, 0.0, 0, 3, 0) == 1
        assert getattr(lib, "amg_residual" + sfx)(1, 1, 0, 0, 0, 0, 0, 0, 128, 0) == 1
        assert getattr(lib, "amg_relax_diag" + sfx)(1, 1, 0, 0, 0, 0, 0, 0, 0, 6, 0) == 1
    assert lib.amg_spmv_c128(1, 1, 0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0, 3, 0) == 1


# ---------------------------------------------------------------------------
# matrices and references
# ---------------------------------------------------------------------------
def _values(rng, n, dt):
    v = rng.standard_normal(n)
    if dt == "c128":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(NP_DTYPE[dt])


def _csr(name, rng):
    """'one': 1x1.  'ragged': 67 rows (no multiple of 64 nor of 256/subw) by
    80 columns; rows 13 and 66 (the last) are empty, row 40 has 70 entries
    (longer than the widest sub-wave, so the strided loop wraps), the others
    1 to 9."""
    if name == "one":
        return 1, np.array([0, 1], np.int32), np.array([0], np.int32)
    n, ncols = 67, 80
    lens = rng.integers(1, 10, size=n)
    lens[[13, 66]] = 0
    lens[40] = 70
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=ptr[1:])
    col = np.concatenate([np.sort(rng.choice(ncols, size=k, replace=False))
                          for k in lens]).astype(np.int32)
    return ncols, ptr, col


def _matvec(ptr, col, val, x):
    acc = np.complex128 if np.iscomplexobj(val) else np.float64
    v, xx = val.astype(acc), x.astype(acc)
    return np.array([np.dot(v[ptr[i]:ptr[i + 1]], xx[col[ptr[i]:ptr[i + 1]]])
                     for i in range(len(ptr) - 1)], dtype=acc)


@pytest.fixture(scope="module")
def cases(hip_backend):
    """(matrix, dtype) -> host arrays, their device copies and A x, computed
    once and never written by a test."""
    import torch

    out = {}
    for mi, mname in enumerate(("one", "ragged")):
        for di, dt in enumerate(NP_DTYPE):
            rng = np.random.default_rng(100 + 10 * mi + di)
            ncols, ptr, col = _csr(mname, rng)
            n = len(ptr) - 1
            c = types.SimpleNamespace(n=n, ncols=ncols, nnz=len(col), ptr=ptr, col=col,
                                      dt=dt, val=_values(rng, len(col), dt),
                                      x=_values(rng, ncols, dt), rhs=_values(rng, n, dt),
                                      y0=_values(rng, n, dt), M=_values(rng, n, dt))
            c.Ax = _matvec(ptr, col, c.val, c.x)
            c.dev = {k: torch.from_numpy(getattr(c, k)).to(hip_backend.device)
                     for k in ("ptr", "col", "val", "x", "rhs", "y0", "M")}
            out[mname, dt] = c
    return out


def _wide(a):
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def _check(got, ref, dt, what):
    got = _wide(got.cpu().numpy())
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    print(f"{what} {dt}: max abs err {err:.3e}")
    if dt == "f32":
        assert err < 1e-4
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def _stream():
    from amgcl_amd.backend.hip import _stream as s

    return s()


ALPHA = {"f64": 1.7, "f32": 1.7, "c128": 1.7 - 0.4j}
BETA = {"f64": 0.3, "f32": 0.3, "c128": 0.3 + 0.6j}


# ---------------------------------------------------------------------------
# CSR row kernels: op x dtype x subw
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("subw", SUBWS)
@pytest.mark.parametrize("dt", list(NP_DTYPE))
@pytest.mark.parametrize("mname", ["one", "ragged"])
@pytest.mark.parametrize("op", ["spmv_beta0", "spmv", "residual", "relax_diag"])
def test_csr_dispatch(cases, op, mname, dt, subw):
    c = cases[mname, dt]
    d = c.dev
    lib = _hiplib.lib()
    A = (c.n, c.nnz, d["ptr"].data_ptr(), d["col"].data_ptr(), d["val"].data_ptr())
    out = d["y0"].clone()
    if op in ("spmv_beta0", "spmv"):
        alpha, beta = ALPHA[dt], (BETA[dt] if op == "spmv" else 0.0)
        if dt == "c128":
            scal = (alpha.real, alpha.imag, complex(beta).real, complex(beta).imag)
        else:
            scal = (alpha, beta)
        rc = getattr(lib, "amg_spmv_" + dt)(*A, d["x"].data_ptr(), *scal, out.data_ptr(),
                                            subw, _stream())
        ref = alpha * c.Ax + beta * _wide(c.y0)
    elif op == "residual":
        rc = getattr(lib, "amg_residual_" + dt)(*A, d["rhs"].data_ptr(), d["x"].data_ptr(),
                                                out.data_ptr(), subw, _stream())
        ref = _wide(c.rhs) - c.Ax
    else:
        rc = getattr(lib, "amg_relax_diag_" + dt)(*A, d["M"].data_ptr(),
                                                  d["rhs"].data_ptr(), d["x"].data_ptr(),
                                                  out.data_ptr(), subw, _stream())
        ref = _wide(c.M) * (_wide(c.rhs) - c.Ax)
    _hiplib.check(rc, op)
    _check(out, ref, dt, f"{op} {mname} subw={subw}")


# ---------------------------------------------------------------------------
# SELL launchers, with and without a row permutation
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sell(cases):
    from amgcl_amd.backend.hip import DeviceCSR

    out = {}
    for dt in ("f64", "f32"):
        c = cases["ragged", dt]
        d = c.dev
        for perm in (False, True):
            A = DeviceCSR.from_tensors(c.n, c.ncols, d["ptr"], d["col"], d["val"])
            if perm:  # force the sigma sort: one 64-row window per slice
                A.build_sell(sigma=64, sigma_min_rows=0, sigma_min_pad=0.0)
                assert A.srows is not None and A.nslice == 2
            else:
                A.build_sell()
                assert A.srows is None and A.nslice == 2
            out[dt, perm] = A
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", ["spmv_beta0", "spmv", "residual", "relax"])
def test_sell_dispatch(cases, sell, op, dt, perm):
    c = cases["ragged", dt]
    d = c.dev
    S = sell[dt, perm]
    lib = _hiplib.lib()
    A = (S.nrows, S.nslice, S.soff.data_ptr(), S.scol.data_ptr(), S.sval.data_ptr(),
         S.srows.data_ptr() if perm else 0)
    out = d["y0"].clone()
    if op in ("spmv_beta0", "spmv"):
        beta = BETA[dt] if op == "spmv" else 0.0
        rc = getattr(lib, "amg_sell_spmv_" + dt)(*A, d["x"].data_ptr(), ALPHA[dt], beta,
                                                 out.data_ptr(), _stream())
        ref = ALPHA[dt] * c.Ax + beta * _wide(c.y0)
    elif op == "residual":
        rc = getattr(lib, "amg_sell_residual_" + dt)(*A, d["rhs"].data_ptr(),
                                                     d["x"].data_ptr(), out.data_ptr(),
                                                     _stream())
        ref = _wide(c.rhs) - c.Ax
    else:  # xn = x + M (rhs - A x); x is longer than the matrix has rows
        rc = getattr(lib, "amg_sell_relax_" + dt)(*A, d["M"].data_ptr(),
                                                  d["rhs"].data_ptr(), d["x"].data_ptr(),
                                                  out.data_ptr(), _stream())
        ref = _wide(c.x[:c.n]) + _wide(c.M) * (_wide(c.rhs) - c.Ax)
    _hiplib.check(rc, op)
    _check(out, ref, dt, f"sell {op} perm={perm}")


# ---------------------------------------------------------------------------
# vector-op pairs: each _f64/_f32 forwarder once
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vecs(hip_backend):
    """(n, dtype) -> host x, y, z, m, a dense n x n matrix, an index
    permutation, and device copies.  Values and the coefficients used below
    are positive: without cancellation the purely relative fp64 bounds hold
    whether or not the compiler fuses a multiply-add."""
    import torch

    out = {}
    for n in (1, 65, 257):
        for di, dt in enumerate(("f64", "f32")):
            rng = np.random.default_rng(200 + 2 * n + di)

            def pos(k):
                return (rng.random(k) + 0.5).astype(NP_DTYPE[dt])

            v = types.SimpleNamespace(n=n, x=pos(n), y=pos(n), z=pos(n), m=pos(n),
                                      a=pos(n * n),
                                      idx=rng.permutation(n).astype(np.int32))
            v.dev = {k: torch.from_numpy(getattr(v, k)).to(hip_backend.device)
                     for k in ("x", "y", "z", "m", "a", "idx")}
            out[n, dt] = v
    return out


def _check_vec(got, ref, dt, rtol, what):
    got = _wide(got.cpu().numpy())
    err = float(np.abs(got - ref).max())
    print(f"{what} {dt}: max abs err {err:.3e}")
    if dt == "f32":
        assert err < 1e-4
    else:
        np.testing.assert_allclose(got, ref, rtol=rtol)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 257])
def test_vector_forwarders(vecs, n, dt):
    import torch

    v = vecs[n, dt]
    d = v.dev
    lib = _hiplib.lib()
    x, y, z, m = (_wide(a) for a in (v.x, v.y, v.z, v.m))

    def fn(name):
        return getattr(lib, f"amg_{name}_{dt}")

    for b in (0.0, 0.5):
        out = d["y"].clone()
        _hiplib.check(fn("axpby")(n, 1.5, d["x"].data_ptr(), b, out.data_ptr(), _stream()),
                      "axpby")
        _check_vec(out, 1.5 * x + b * y, dt, 1e-13, f"axpby b={b}")
    for c in (0.0, 1.1):
        out = d["z"].clone()
        _hiplib.check(fn("axpbypcz")(n, 0.3, d["x"].data_ptr(), 0.7, d["y"].data_ptr(), c,
                                     out.data_ptr(), _stream()), "axpbypcz")
        _check_vec(out, 0.3 * x + 0.7 * y + c * z, dt, 1e-12, f"axpbypcz c={c}")
    for b in (0.0, 0.25):
        out = d["z"].clone()
        _hiplib.check(fn("vmul")(n, 2.0, d["m"].data_ptr(), d["x"].data_ptr(), b,
                                 out.data_ptr(), _stream()), "vmul")
        _check_vec(out, 2.0 * m * x + b * z, dt, 1e-13, f"vmul b={b}")

    out = d["z"].clone()
    _hiplib.check(fn("fill")(n, 0.375, out.data_ptr(), _stream()), "fill")
    assert np.all(out.cpu().numpy() == 0.375)

    dot = torch.full((2,), 7.0, dtype=torch.float64, device=d["x"].device)
    _hiplib.check(fn("dot")(n, d["x"].data_ptr(), d["y"].data_ptr(), dot.data_ptr(),
                            _stream()), "dot")
    err = abs(float(dot[0].item()) - float(np.dot(x, y)))
    print(f"dot {dt}: abs err {err:.3e}")
    assert err < (1e-3 if dt == "f32" else 1e-7 * n**0.5)
    assert float(dot[1].item()) == 7.0  # one result slot, the next is untouched

    out = torch.zeros_like(d["x"])
    _hiplib.check(fn("gather")(n, d["x"].data_ptr(), d["idx"].data_ptr(), out.data_ptr(),
                               _stream()), "gather")
    np.testing.assert_array_equal(out.cpu().numpy(), v.x[v.idx])
    out = torch.zeros_like(d["x"])
    _hiplib.check(fn("scatter")(n, d["x"].data_ptr(), d["idx"].data_ptr(), out.data_ptr(),
                                _stream()), "scatter")
    ref = np.zeros_like(v.x)
    ref[v.idx] = v.x
    np.testing.assert_array_equal(out.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 65])
def test_gemv_forwarders(vecs, n, dt):
    import torch

    v = vecs[n, dt]
    d = v.dev
    out = torch.zeros_like(d["x"])
    _hiplib.check(getattr(_hiplib.lib(), "amg_gemv_" + dt)(
        n, d["a"].data_ptr(), d["x"].data_ptr(), out.data_ptr(), _stream()), "gemv")
    ref = _wide(v.a).reshape(n, n) @ _wide(v.x)
    _check(out, ref, dt, f"gemv n={n}")
