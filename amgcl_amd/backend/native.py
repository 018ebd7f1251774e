"""Native solve driver bindings.

Hands the whole AMG-preconditioned CG/BiCGStab solve to the C++ driver
(csrc/hip/driver.hip) — one ctypes call per solve, no Python in the hot
path. Engaged automatically by make_solver for HIP-backend AMG with diagonal
smoothers (SPAI0/damped Jacobi), Chebyshev, ILU0 with the iterated-Jacobi
solve or SPAI-1, dense-inverse coarse solve (or the smoother on the coarsest
level), and cg/bicgstab; anything else uses the generic Python orchestration.
"""
import ctypes

from ._hiplib import lib as _lib


class OpDescC(ctypes.Structure):
    _fields_ = [
        ("nrows", ctypes.c_int64),
        ("nnz", ctypes.c_int64),
        ("ptr", ctypes.c_void_p),
        ("col", ctypes.c_void_p),
        ("val", ctypes.c_void_p),
        ("subw", ctypes.c_int),
        ("nslice", ctypes.c_int64),
        ("soff", ctypes.c_void_p),
        ("scol", ctypes.c_void_p),
        ("sval", ctypes.c_void_p),
        ("srows", ctypes.c_void_p),
        ("smask", ctypes.c_void_p),
        ("moff", ctypes.c_void_p),
    ]


class LevelDescC(ctypes.Structure):
    _fields_ = [
        ("A", OpDescC),
        ("P", OpDescC),
        ("R", OpDescC),
        ("M", ctypes.c_void_p),
        ("f", ctypes.c_void_p),
        ("u", ctypes.c_void_p),
        ("t", ctypes.c_void_p),
        ("cheb_degree", ctypes.c_int),
        ("cheb_theta", ctypes.c_double),
        ("cheb_delta", ctypes.c_double),
        ("cheb_sigma1", ctypes.c_double),
        ("cheb_d", ctypes.c_void_p),
        ("bsize", ctypes.c_int),
        ("nbrows", ctypes.c_int64),
        ("bptr", ctypes.c_void_p),
        ("bcol", ctypes.c_void_p),
        ("bval", ctypes.c_void_p),
        ("spai1", OpDescC),
        ("ilu_iters", ctypes.c_int),
        ("ilu_damping", ctypes.c_double),
        ("ilu_jdamping", ctypes.c_double),
        ("ilu_L", OpDescC),
        ("ilu_U", OpDescC),
        ("ilu_dinv", ctypes.c_void_p),
        ("ilu_y", ctypes.c_void_p),
        ("ilu_s", ctypes.c_void_p),
        ("ilu_b", ctypes.c_void_p),
    ]


def desc_layout():
    """[(label, value)]: both struct sizes, then every OpDescC and LevelDescC
    field offset, in the order the library's amg_desc_layout reports them."""
    out = [("sizeof(OpDesc)", ctypes.sizeof(OpDescC)),
           ("sizeof(LevelDesc)", ctypes.sizeof(LevelDescC))]
    for cls in (OpDescC, LevelDescC):
        out += [(f"offsetof({cls.__name__[:-1]}, {name})", getattr(cls, name).offset)
                for name, _ in cls._fields_]
    return out


def lib_desc_layout(L):
    """The same list as the compiled library has it."""
    buf = (ctypes.c_int64 * 64)()
    count = L.amg_desc_layout(buf, len(buf))
    return list(buf[:min(count, len(buf))])


_driver_bound = False


def _bind():
    global _driver_bound
    L = _lib()
    if not _driver_bound:
        # OpDescC / LevelDescC above are hand-kept copies of the C structs
        # (amg_common.h): refuse to pass them on if the two sides disagree on
        # a size or on where any field sits
        ours, theirs = desc_layout(), lib_desc_layout(L)
        if len(ours) != len(theirs):
            raise RuntimeError(
                f"descriptor layout mismatch: libamghip.so reports {len(theirs)} "
                f"entries, backend/native.py has {len(ours)}")
        for (label, mine), lib_value in zip(ours, theirs):
            if mine != lib_value:
                raise RuntimeError(
                    f"descriptor layout mismatch at {label}: libamghip.so has "
                    f"{lib_value}, backend/native.py has {mine}")
        L.amg_driver_create.argtypes = [
            ctypes.POINTER(LevelDescC), ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(OpDescC), ctypes.c_void_p,
        ]
        L.amg_driver_create.restype = ctypes.c_void_p
        L.amg_driver_destroy.argtypes = [ctypes.c_void_p]
        L.amg_driver_destroy.restype = None
        L.amg_driver_cg.argtypes = (
            [ctypes.c_void_p] + [ctypes.c_void_p] * 7
            + [ctypes.c_double, ctypes.c_double, ctypes.c_int,
               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
        )
        L.amg_driver_cg.restype = ctypes.c_int
        L.amg_driver_bicgstab.argtypes = (
            [ctypes.c_void_p] + [ctypes.c_void_p] * 10
            + [ctypes.c_double, ctypes.c_double, ctypes.c_int,
               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
        )
        L.amg_driver_bicgstab.restype = ctypes.c_int
        L.amg_driver_precond.argtypes = [ctypes.c_void_p] * 4
        L.amg_driver_precond.restype = ctypes.c_int
        _driver_bound = True
    return L


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _op(dst, M, keep, subw=None):
    """Fill the OpDescC dst from the DeviceCSR M (CSR arrays, plus the SELL
    image, padded with its sigma permutation or compact with its masks, when
    M has one) and append every tensor
    it now points at to keep.  subw overrides M's own; 0 lets the driver
    choose."""
    dst.nrows, dst.nnz = M.nrows, int(M.nnz)
    dst.ptr, dst.col, dst.val = _ptr(M.ptr), _ptr(M.col), _ptr(M.val)
    dst.subw = M.subw if subw is None else subw
    keep.extend([M.ptr, M.col, M.val])
    if getattr(M, "nslice", 0):
        dst.nslice = M.nslice
        dst.soff, dst.scol, dst.sval = _ptr(M.soff), _ptr(M.scol), _ptr(M.sval)
        dst.srows = _ptr(M.srows)
        dst.smask, dst.moff = _ptr(M.smask), _ptr(M.moff)
        keep.extend([M.soff, M.scol, M.sval, M.srows, M.smask, M.moff])


class NativeDriver:
    """Owns the C driver handle plus references to every device tensor it
    points at (torch would otherwise free them under the caching allocator)."""

    def __init__(self, amg, backend, solver_kind="cg", solver_prm=None):
        import torch

        from ..relaxation.chebyshev import Chebyshev
        from ..relaxation.ilu0 import ILU0
        from ..relaxation.spai0 import DiagonalSmootherBase, Spai1
        from .hip import DeviceBSR, DeviceCSR, DeviceDenseSolver

        self.backend = backend
        self.solver_kind = solver_kind
        solver_prm = solver_prm or {"tol": 1e-8, "abstol": 0.0, "maxiter": 100}
        self.tol = float(solver_prm["tol"])
        self.abstol = float(solver_prm["abstol"])
        self.maxiter = int(solver_prm["maxiter"])

        levels = amg.levels
        if not all(isinstance(l.A, (DeviceCSR, DeviceBSR)) for l in levels):
            raise TypeError("native driver needs device-resident levels")
        self._mixed = bool(getattr(amg, "_mixed", False))
        def relax_ok(r):
            if isinstance(r, (DiagonalSmootherBase, Chebyshev, Spai1)):
                return True
            # ILU0 with the iterated-Jacobi solve (graph-capturable); the
            # exact cooperative sptrsv stays on the generic path
            return (isinstance(r, ILU0) and not getattr(r, "_serial", True)
                    and not getattr(r, "_exact", False))

        for l in levels[:-1]:
            if not relax_ok(l.relax):
                raise TypeError(
                    "native driver supports diagonal/Chebyshev/ILU0(jacobi)/SPAI-1")
        if amg.coarse_solve is not None and not isinstance(
            amg.coarse_solve, DeviceDenseSolver
        ):
            raise TypeError("native driver needs the dense coarse solver")
        if amg.coarse_solve is None and not relax_ok(levels[-1].relax):
            raise TypeError("native coarsest smoother unsupported")

        keep = self._keep = []  # tensor refs
        descs = (LevelDescC * len(levels))()
        n0 = levels[0].A.nrows
        for i, l in enumerate(levels):
            d = descs[i]
            A = l.A
            if isinstance(A, DeviceBSR):
                d.A.nrows, d.A.nnz = A.nrows, int(A.nnz)
                d.bsize, d.nbrows = A.bsize, A.nbrows
                d.bptr, d.bcol, d.bval = _ptr(A.ptr), _ptr(A.col), _ptr(A.val)
                keep.extend([A.ptr, A.col, A.val])
            else:
                _op(d.A, A, keep)
            if l.P is not None:
                _op(d.P, l.P, keep)
                _op(d.R, l.R, keep)
            relax = l.relax
            if isinstance(relax, ILU0):
                d.ilu_iters = relax.solve_iters
                d.ilu_damping = relax.damping
                d.ilu_jdamping = relax.solve_damping
                # subw 2: the width the triangular sweeps have always run with
                _op(d.ilu_L, relax.L, keep, subw=2)
                _op(d.ilu_U, relax.U, keep, subw=2)
                d.ilu_dinv = _ptr(relax.Dinv)
                work = [torch.empty(A.nrows, dtype=torch.float64,
                                    device=backend.device) for _ in range(3)]
                d.ilu_y, d.ilu_s, d.ilu_b = (_ptr(work[0]), _ptr(work[1]),
                                             _ptr(work[2]))
                keep.extend([relax.Dinv] + work)
            elif isinstance(relax, Chebyshev):
                d.cheb_degree = relax.degree
                d.cheb_theta = relax.theta
                d.cheb_delta = relax.delta
                d.cheb_sigma1 = relax.sigma1
                cheb_d = torch.empty(A.nrows, dtype=torch.float64,
                                     device=backend.device)
                d.cheb_d = _ptr(cheb_d)
                keep.append(cheb_d)
                d.M = _ptr(relax.Dinv)  # optional D^-1 scaling (may be null)
                if relax.Dinv is not None:
                    keep.append(relax.Dinv)
            elif isinstance(relax, Spai1):
                _op(d.spai1, relax.M, keep)
            elif relax is not None:
                d.M = _ptr(relax.M)
                keep.append(relax.M)
            d.f = _ptr(l.f)
            d.u = _ptr(l.u)
            d.t = _ptr(l.t)
            keep.extend([l.f, l.u, l.t])

        inv = amg.coarse_solve.inv if amg.coarse_solve is not None else None
        if inv is not None:
            keep.append(inv)
        prm = amg.prm
        L = _bind()
        stream = torch.cuda.current_stream().cuda_stream
        a64 = None
        if self._mixed:
            # the Krylov loop keeps iterating with the fp64 fine operator;
            # the LevelDescs above point at the fp32 hierarchy for the cycle
            a64 = OpDescC()
            _op(a64, amg._A64, keep)
        self.handle = L.amg_driver_create(
            descs, len(levels), _ptr(inv),
            amg.coarse_solve.n if amg.coarse_solve is not None else 0,
            int(prm["npre"]), int(prm["npost"]), int(prm["ncycle"]),
            int(prm["pre_cycles"]), int(self._mixed), a64, ctypes.c_void_p(stream),
        )
        if not self.handle:
            raise RuntimeError("amg_driver_create failed")
        nwork = 5 if solver_kind == "cg" else 8
        self._work = [torch.empty(n0, dtype=torch.float64, device=backend.device)
                      for _ in range(nwork)]
        self._descs = descs

    def solve(self, rhs, x):
        L = _bind()
        iters = ctypes.c_int64(0)
        resid = ctypes.c_double(0.0)
        w = [_ptr(t) for t in self._work]
        if self.solver_kind == "cg":
            rc = L.amg_driver_cg(self.handle, _ptr(rhs), _ptr(x), *w, self.tol,
                                 self.abstol, self.maxiter,
                                 ctypes.byref(iters), ctypes.byref(resid))
        else:
            rc = L.amg_driver_bicgstab(self.handle, _ptr(rhs), _ptr(x), *w, self.tol,
                                       self.abstol, self.maxiter,
                                       ctypes.byref(iters), ctypes.byref(resid))
        if rc != 0:
            raise RuntimeError(f"native solve failed rc={rc}")
        return int(iters.value), float(resid.value)

    def precond_apply(self, rhs, x):
        """x = M^-1 rhs (one native V-cycle stack application)."""
        L = _bind()
        rc = L.amg_driver_precond(self.handle, _ptr(rhs), _ptr(x), _ptr(self._work[0]))
        if rc != 0:
            raise RuntimeError(f"native precond failed rc={rc}")

    def __del__(self):
        try:
            _bind().amg_driver_destroy(self.handle)
        except Exception:
            pass


def try_native(make_solver_obj):
    """Attach a native driver to a MakeSolver when the configuration allows;
    returns None otherwise."""
    from ..precond.amg import AMG
    from ..solver.bicgstab import BiCGStab
    from ..solver.cg import CG

    P, S, backend = make_solver_obj.P, make_solver_obj.S, make_solver_obj.backend
    if getattr(backend, "name", "") != "hip":
        return None
    if "complex" in str(getattr(backend, "dtype", "")):
        return None  # complex solves use the generic per-kernel path
    if not isinstance(P, AMG):
        return None
    if isinstance(S, CG):
        kind = "cg"
    elif isinstance(S, BiCGStab) and S.prm["pside"] == "right" and not S.prm["check_after"]:
        kind = "bicgstab"
    else:
        return None
    if S.prm.get("verbose") or S.prm.get("ns_search"):
        return None
    try:
        return NativeDriver(P, backend, kind, S.prm)
    except TypeError:
        return None
