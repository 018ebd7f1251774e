"""The compact (pad-free) SELL-64 image: its layout, its three kernel modes,
the rule that chooses it, and the native driver and torch-free C API on it.

Layout (csrc/hip/kernels.hip): slice = 64 consecutive rows, lane = row, slot
i = the row's i-th CSR entry; a slot stores only the lanes whose row is longer
than i, packed in lane order, with one 64-bit lane mask per slot in smask.
moff[s] .. moff[s+1] are slice s's masks and its entries start at the CSR
ptr[64 s].
"""
import os
import types

import numpy as np
import pytest

import amgcl_amd as am
from amgcl_amd.backend import _hiplib

SIZES = [1, 63, 64, 65, 200]
PATTERNS = ["equal", "alt15", "decreasing", "increasing", "empty", "long"]
NP_DTYPE = {"f64": np.float64, "f32": np.float32}
ALPHA, BETA = 1.7, 0.3
U53, U24 = 2.0 ** -53, 2.0 ** -24


def _lens(pattern, n):
    i = np.arange(n)
    if pattern == "equal":  # every mask of a full slice is full
        return np.full(n, 4)
    if pattern == "alt15":  # the active lanes of slots 1..4 are not contiguous
        return np.where(i % 2 == 0, 1, 5)
    if pattern == "decreasing":  # strictly, within each slice
        return 64 - i % 64
    if pattern == "increasing":
        return 1 + i % 64
    if pattern == "empty":  # empty rows; rows 64..127 are one all-empty slice
        lens = np.where(i % 3 == 0, 0, 1 + i % 4)
        lens[64:128] = 0
        return lens
    lens = np.ones(n, dtype=np.int64)  # "long": more slots than lanes
    lens[min(40, n - 1)] = 130
    return lens


def _ncols(n):
    # rectangular like P and R, wide enough for a 130-entry row and for the
    # relax mode's x[row]
    return max(n + 37, 160)


def _row_sums(ptr, col, val, x):
    """A x and sum |a_ij||x_j| per row, in extended precision (the reference
    must not carry rounding errors of the size the bound allows the kernel)."""
    v, xx = val.astype(np.longdouble), x.astype(np.longdouble)
    n = len(ptr) - 1
    ax, aax = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
    for i in range(n):
        p = v[ptr[i]:ptr[i + 1]] * xx[col[ptr[i]:ptr[i + 1]]]
        ax[i], aax[i] = p.sum(), np.abs(p).sum()
    return ax, aax


@pytest.fixture(scope="module")
def cases(hip_backend):
    """(n, pattern, dtype) -> host arrays, device copies, the compact and the
    padded image and the float64 reference; built once, never written."""
    import torch

    from amgcl_amd.backend.hip import DeviceCSR

    out = {}
    for n in SIZES:
        for pi, pattern in enumerate(PATTERNS):
            for di, dt in enumerate(NP_DTYPE):
                rng = np.random.default_rng(1000 * n + 10 * pi + di)
                lens, ncols, npdt = _lens(pattern, n), _ncols(n), NP_DTYPE[dt]
                ptr = np.zeros(n + 1, np.int32)
                np.cumsum(lens, out=ptr[1:])
                col = np.concatenate(
                    [np.sort(rng.choice(ncols, size=k, replace=False)) for k in lens]
                    + [np.zeros(0, np.int64)]).astype(np.int32)
                rnd = lambda m: rng.standard_normal(m).astype(npdt)
                c = types.SimpleNamespace(n=n, ncols=ncols, lens=lens, ptr=ptr, col=col,
                                          val=rnd(len(col)), x=rnd(ncols), rhs=rnd(n),
                                          y0=rnd(n), M=rnd(n))
                c.Ax, c.absAx = _row_sums(ptr, col, c.val, c.x)
                c.dev = {k: torch.from_numpy(getattr(c, k)).to(hip_backend.device)
                         for k in ("ptr", "col", "val", "x", "rhs", "y0", "M")}
                d = c.dev
                mk = lambda: DeviceCSR.from_tensors(n, ncols, d["ptr"], d["col"], d["val"])
                c.compact = mk().build_sell(compact=True)
                c.padded = mk().build_sell()
                assert c.compact.smask is not None and c.compact.soff is None
                assert c.padded.smask is None and c.padded.soff is not None
                assert c.compact.nslice == c.padded.nslice == (n + 63) // 64
                out[n, pattern, dt] = c
    return out


def _stream():
    from amgcl_amd.backend.hip import _stream as s

    return s()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(NP_DTYPE))
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_compact_image(cases, n, pattern, dt):
    """Unpacking scol/sval through smask/moff gives back the CSR col/val bit
    for bit; there is one mask per slot of every slice and a slice's masks
    hold as many bits as the slice has entries."""
    c = cases[n, pattern, dt]
    S = c.compact
    moff = S.moff.cpu().numpy()
    smask = S.smask.cpu().numpy().view(np.uint64)
    scol, sval = S.scol.cpu().numpy(), S.sval.cpu().numpy()
    nslice = S.nslice
    assert moff.shape == (nslice + 1,) and moff[0] == 0
    assert scol.shape == c.col.shape and sval.shape == c.val.shape
    assert sval.dtype == c.val.dtype
    lens = np.concatenate([c.lens, np.zeros(nslice * 64 - n, dtype=c.lens.dtype)])
    widths = lens.reshape(nslice, 64).max(axis=1)
    assert np.array_equal(np.diff(moff), widths)
    assert moff[-1] == widths.sum() and smask.size == max(widths.sum(), 1)
    if pattern == "empty" and n > 64:
        assert widths[1] == 0
    ucol = np.full_like(c.col, -1)
    uval = np.full_like(c.val, np.nan)
    for s in range(nslice):
        off = int(c.ptr[64 * s])
        bits = 0
        for i in range(int(moff[s]), int(moff[s + 1])):
            m = int(smask[i])
            slot = i - int(moff[s])
            want = sum(1 << l for l in range(64) if lens[64 * s + l] > slot)
            assert m == want, (s, slot)
            rank = 0
            for lane in range(64):
                if (m >> lane) & 1:
                    dst = int(c.ptr[64 * s + lane]) + slot
                    ucol[dst], uval[dst] = scol[off + rank], sval[off + rank]
                    rank += 1
            off += rank
            bits += rank
        assert bits == int(c.ptr[min(64 * (s + 1), n)]) - int(c.ptr[64 * s])
    assert np.array_equal(ucol, c.col)
    assert ucol.tobytes() == c.col.tobytes() and uval.tobytes() == c.val.tobytes()


def _run(S, op, dt, d):
    """One kernel mode through the entry point of S's image family."""
    lib = _hiplib.lib()
    out = d["y0"].clone()
    name = S.sell_name
    if op in ("spmv_beta0", "spmv"):
        rc = getattr(lib, f"amg_{name}_spmv_{dt}")(
            *S.sell_args, d["x"].data_ptr(), ALPHA, BETA if op == "spmv" else 0.0,
            out.data_ptr(), _stream())
    elif op == "residual":
        rc = getattr(lib, f"amg_{name}_residual_{dt}")(
            *S.sell_args, d["rhs"].data_ptr(), d["x"].data_ptr(), out.data_ptr(),
            _stream())
    else:
        rc = getattr(lib, f"amg_{name}_relax_{dt}")(
            *S.sell_args, d["M"].data_ptr(), d["rhs"].data_ptr(), d["x"].data_ptr(),
            out.data_ptr(), _stream())
    _hiplib.check(rc, op)
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(NP_DTYPE))
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_compact_kernels(cases, n, pattern, dt):
    """y = aAx (+ by), r = rhs - Ax and xn = x + M(rhs - Ax) on the compact
    image against the host reference (float64 data, evaluated in extended
    precision).

    Bound per row, first order in u = 2^-53.  The row sum is a dot product of
    len terms accumulated in double: (len + 2) u sum|a_ij||x_j| = E.  Each
    operation of the epilogue adds u times the magnitude it produces, taken
    over the operands so that a reassociated form (fast-math) is covered:
      y  = a s + b y0         |a| E + u (|a s| + |b y0| + |y|)
      r  = rhs - s            E + u |r|
      xn = x + M (rhs - s)    |M| E + u (2 |M| (|rhs| + |s|) + |xn|)
    A float output adds the final rounding 2^-24 |result|.  The count of
    outputs bit-identical to the padded kernel's is printed, not asserted."""
    c = cases[n, pattern, dt]
    w = lambda a: a.astype(np.longdouble)
    E = (c.lens + 2) * U53 * c.absAx
    rhs, x, M, y0 = w(c.rhs), w(c.x[:n]), w(c.M), w(c.y0)
    refs = {
        "spmv_beta0": (ALPHA * c.Ax,
                       ALPHA * E + U53 * 2 * np.abs(ALPHA * c.Ax)),
        "spmv": (ALPHA * c.Ax + BETA * y0,
                 ALPHA * E + U53 * (np.abs(ALPHA * c.Ax) + np.abs(BETA * y0)
                                    + np.abs(ALPHA * c.Ax + BETA * y0))),
        "residual": (rhs - c.Ax, E + U53 * np.abs(rhs - c.Ax)),
        "relax": (x + M * (rhs - c.Ax),
                  np.abs(M) * E + U53 * (2 * np.abs(M) * (np.abs(rhs) + np.abs(c.Ax))
                                         + np.abs(x + M * (rhs - c.Ax)))),
    }
    failures = []
    for op, (ref, bound) in refs.items():
        got_raw = _run(c.compact, op, dt, c.dev)
        pad_raw = _run(c.padded, op, dt, c.dev)
        got = w(got_raw)
        if dt == "f32":
            bound = bound + U24 * np.abs(ref)
        err = np.abs(got - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0
        same = int((got_raw.view(np.uint8).reshape(n, -1)
                    == pad_raw.view(np.uint8).reshape(n, -1)).all(axis=1).sum())
        print(f"compact {op} n={n} {pattern} {dt}: max err/bound {worst:.3f}, "
              f"bit-identical to padded {same}/{n}")
        if not (err <= bound).all():
            failures.append((op, worst))
    assert not failures, failures


@pytest.mark.gpu
def test_compact_backend_dispatch(hip_backend, cases):
    """HipBackend.spmv / residual / relax_diag pick the compact kernels for a
    matrix that carries the compact image, and bytes() counts its arrays."""
    import torch

    c = cases[200, "alt15", "f64"]
    S, d = c.compact, c.dev
    y = d["y0"].clone()
    hip_backend.spmv(ALPHA, S, d["x"], BETA, y)
    assert np.array_equal(y.cpu().numpy(), _run(S, "spmv", "f64", d))
    r = torch.empty_like(y)
    hip_backend.residual(d["rhs"], S, d["x"], r)
    assert np.array_equal(r.cpu().numpy(), _run(S, "residual", "f64", d))
    xx, t = d["x"].clone(), torch.empty(c.ncols, dtype=torch.float64, device=y.device)
    t[:] = d["x"]
    hip_backend.relax_diag(S, d["M"], d["rhs"], xx, t)
    assert np.array_equal(xx.cpu().numpy()[:c.n], _run(S, "relax", "f64", d))
    nnz = len(c.col)
    csr = (c.n + 1 + nnz) * 4 + nnz * 8
    assert S.bytes() == csr + nnz * 12 + (S.smask.numel() + S.nslice + 1) * 8
    P = c.padded
    assert P.bytes() == csr + P.scol.numel() * 12 + (P.nslice + 1) * 8


def _rule(rows, mean, pad, vbytes=8):
    """The exported rule on an operator given by its row count, mean row
    length and SELL-64 padding factor (padded slots / nnz)."""
    nnz = int(round(rows * mean))
    nmask = int(round(pad * nnz / 64))
    return bool(_hiplib.lib().amg_sell_compact_rule(
        nmask * 64, nnz, nmask, (rows + 63) // 64, vbytes))


def test_compact_rule():
    """Compact exactly when the padding bytes it removes exceed the bytes of
    masks and offsets it adds: uniform rows stay padded, the alternating 1/5
    pattern goes compact, and of the 96^3 hierarchy (rows, mean nnz/row,
    padding factor as measured) only the fine-level A stays padded."""
    rule = _hiplib.lib().amg_sell_compact_rule
    for vbytes in (8, 4):
        # 6400 rows of 7: no padding at all
        assert not rule(100 * 7 * 64, 6400 * 7, 100 * 7, 100, vbytes)
        # 6400 rows alternating 1 and 5: width 5, 3 entries per row
        assert rule(100 * 5 * 64, 6400 * 3, 100 * 5, 100, vbytes)
        assert not _rule(884736, 6.94, 1.004, vbytes)      # A0
        for rows, mean, pad in [(884736, 3.41, 1.53),       # P0
                                (79876, 37.8, 1.52),        # R0
                                (79876, 32.1, 1.33),        # A1
                                (79876, 4.26, 1.77),        # P1
                                (5575, 61.0, 1.60),         # R1
                                (5575, 68.0, 1.35)]:        # A2
            assert _rule(rows, mean, pad, vbytes), (rows, mean, pad)
    # at the boundary: 12 bytes per padding slot against 8 per mask and 8 per
    # offset (one slice of width 2: 16 + 16)
    assert rule(128, 126, 2, 1, 8) == 0   # 2 * 12 = 24 < 32
    assert rule(128, 125, 2, 1, 8) == 1   # 3 * 12 = 36 > 32


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_compact_native_driver(hip_backend, solver):
    """The poisson3d(24) SELL case of test_native_storage_matrix, once with
    the compact image forced on every operator that gets a SELL image and
    once with the padded one, both through the native driver, under that
    test's criteria: CG iteration counts within 1, BiCGStab counts equal,
    res < tol, true residual < 10 tol."""
    A, b = am.poisson3d(24, rhs="random")
    tol = 1e-8
    runs = {}
    for compact in (True, False):
        prm = {"precond": {"class": "amg", "coarse_enough": 300, "sell": "auto",
                           "sell_min_rows": 1, "sell_min_mean": 0.0,
                           "sell_compact": compact},
               "solver": {"type": solver, "tol": tol, "maxiter": 100}}
        s = am.make_solver(A, prm, backend=hip_backend)
        assert s._native is not None
        ops = [M for l in s.P.levels for M in (l.A, l.P, l.R) if M is not None]
        assert len(s.P.levels) >= 2 and all(M.nslice for M in ops)
        assert all((M.smask is not None) == compact for M in ops)
        l0 = s.P.levels[0]
        assert (l0.P.smask is not None) == compact and (l0.R.smask is not None) == compact
        x, it, res = s(b)
        true = np.linalg.norm(b - A @ hip_backend.to_host(x)) / np.linalg.norm(b)
        print(f"compact={compact} {solver}: {it} it, res {res:.3e}, true {true:.3e}")
        assert res < tol and true < 10 * tol
        runs[compact] = it
    if solver == "cg":
        assert abs(runs[True] - runs[False]) <= 1, runs
    else:
        assert runs[True] == runs[False], runs


@pytest.mark.gpu
def test_compact_capi_device_setup(tmp_path):
    """build_sell_capi takes the compact branch at test size: Poisson 24^3
    with precond.sell_min_rows=1 on the torch-free device setup, against the
    same run with AMGCL_SELL_PADDED=1.  The two differ only in the image the
    kernels read."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    A, _ = am.poisson3d(24)
    npz = str(tmp_path / "a24.npz")
    np.savez(npz, ptr=np.asarray(A.ptr, dtype=np.int32),
             col=np.asarray(A.col, dtype=np.int32),
             val=np.asarray(A.val, dtype=np.float64))
    prog = r"""
import ctypes, os, sys
import numpy as np
d = np.load(r"%s")
ptr, col, val = d["ptr"], d["col"], d["val"]
n = len(ptr) - 1
lib = ctypes.CDLL(r"%s/amgcl_amd/_hip/libamghip.so")
lib.amgcl_amd_gpu_solver_create.restype = ctypes.c_void_p
lib.amgcl_amd_gpu_solver_create.argtypes = [ctypes.c_int] + [ctypes.c_void_p]*3 + [ctypes.c_char_p]
lib.amgcl_amd_gpu_solver_solve.restype = ctypes.c_int
lib.amgcl_amd_gpu_solver_solve.argtypes = [ctypes.c_void_p]*3 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
lib.amgcl_amd_gpu_solver_destroy.argtypes = [ctypes.c_void_p]
b = np.ones(n)
cfg = ("solver.type=cg;solver.tol=1e-8;precond.coarse_enough=300;"
       "precond.device_handoff=500;precond.setup=device;precond.sell_min_rows=1")
def run(name):
    print("RUN", name, flush=True)
    h = lib.amgcl_amd_gpu_solver_create(n, ptr.ctypes.data, col.ctypes.data,
                                        val.ctypes.data, cfg.encode())
    assert h, "create failed"
    x = np.zeros(n); it = ctypes.c_int(0); res = ctypes.c_double(0.0)
    rc = lib.amgcl_amd_gpu_solver_solve(h, b.ctypes.data, x.ctypes.data,
                                        ctypes.byref(it), ctypes.byref(res))
    lib.amgcl_amd_gpu_solver_destroy(h)
    assert rc == 0, (name, rc)
    assert res.value < 1e-8, (name, res.value)
    return x, it.value
xc, itc = run("compact")
os.environ["AMGCL_SELL_PADDED"] = "1"
xp, itp = run("padded")
diff = np.linalg.norm(xc - xp) / np.linalg.norm(xp)
print("FIGURES iters compact/padded", itc, itp, "diff", diff, flush=True)
assert itc == itp, (itc, itp)
assert diff < 1e-8, diff
assert "torch" not in sys.modules
print("COMPACT_SETUP_OK", flush=True)
""" % (npz, root)
    env = dict(os.environ, AMGCL_CAPI_TRACE="1")
    env.pop("AMGCL_SELL_PADDED", None)
    out = subprocess.check_output([sys.executable, "-c", prog], text=True, env=env,
                                  stderr=subprocess.STDOUT, timeout=300)
    print(out)
    assert "COMPACT_SETUP_OK" in out
    runs = {}
    for chunk in out.split("RUN ")[1:]:
        name, _, body = chunk.partition("\n")
        runs[name.strip()] = body
    count = lambda name, what: runs[name].count("[capi setup] %s" % what)
    # at least one device-built level, three images each (A, P, R)
    assert count("compact", "sell_compact ") >= 3
    assert count("compact", "sell_compact ") == count("padded", "sell_compact ")
    # P and R of every device-built level go compact by the rule
    assert count("compact", "sell_compact 1 ") >= 2 * count("compact", "record ")
    assert count("compact", "record ") >= 1
    assert count("padded", "sell_compact 1 ") == 0
