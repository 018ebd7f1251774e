"""Distributed AMG hierarchy (cross-rank coarse levels).

Parity: amgcl/mpi/amg.hpp (one AMG hierarchy over the whole distributed
matrix, coarse operators are themselves distributed matrices) with
mpi/coarsening/smoothed_aggregation.hpp semantics. Differences by design:

- Aggregation is rank-local (decoupled) by default: aggregates never cross
  rank boundaries, so P and R are block-diagonal over ranks and the grid
  transfers need no communication — the xGMI-friendly choice (transfers are
  the inner, latency-sensitive ops of the V-cycle). With
  coarsening.cross_rank=True the aggregation instead runs the distributed
  pmis of `parallel/pmis.py` (reference mpi/coarsening/pmis.hpp semantics,
  reproduces the single-process MIS exactly); transfers then halo-exchange.
- The Galerkin product IS fully coupled: Ac = P^T (A_loc P_loc +
  A_rem P_ghost) where the P rows of ghost columns are fetched from their
  owners over the matrix's established comm pattern (the same remote-rows
  exchange as mpi/coarsening/detail galerkin, reference pmis.hpp:149-231).
  Each coarse operator is a genuine DistMatrix with its own halo exchange.
- Coarse levels repartition by REPLICATION: once the global problem fits
  `repart_threshold`, every rank gathers the strips and continues the SAME
  hierarchy serially (a replicated AMG tail, applied redundantly — the
  merge-to-fewer-ranks semantics of mpi/partition/merge.hpp without
  subcommunicator bookkeeping; one all_gather of the level rhs per cycle).
  At `coarse_enough` the replicated tail bottoms out in the dense inverse.

Smoothing runs on the distributed operator (halo exchange + fused local
kernels): SPAI0 / damped Jacobi weights are computed from the FULL row
(local + remote entries).
"""
import numpy as np

from .. import _core
from ..matrix import CSR
from ..params import merge_params
from .dist_matrix import DistMatrix


class _Level:
    __slots__ = ("A", "P", "R", "M", "f", "u", "t", "n_loc")


class DistAMG:
    @staticmethod
    def defaults():
        return {
            "coarsening": {"type": "smoothed_aggregation", "eps_strong": 0.08,
                           "cross_rank": False},  # True: pmis over the halo
            "relax": {"type": "spai0", "damping": 0.72},
            "npre": 1,
            "npost": 1,
            "ncycle": 1,
            "coarse_enough": 3000,
            "repart_threshold": 20000,  # replicate the hierarchy below this
            "max_levels": 20,
            # >1: only every coarse_group_size-th rank (the group master)
            # builds and applies the coarse tail; slaves receive the solution
            # by an intra-group broadcast.  Parity role:
            # amgcl/mpi/direct_solver/solver_base.hpp:69-163
            # (slaves_per_master comm split) — tail memory O(n^2) only on
            # masters instead of every rank.
            "coarse_group_size": 1,
            # coarse direct solver on the master ranks: "dense" (device
            # GEMV inverse), "skyline" (profile LU) or "splu"
            "direct_solver": "dense",
        }

    def __init__(self, dist_A: DistMatrix, prm=None, backend=None):
        import torch.distributed as dist

        self.prm = merge_params(self.defaults(), prm)
        if self.prm["coarsening"]["type"] != "smoothed_aggregation":
            raise ValueError("dist_amg supports smoothed_aggregation coarsening")
        self.backend = backend  # DistBackend
        self.base = backend.base if hasattr(backend, "base") else backend
        self.dist = dist
        self.group = dist_A.group
        self.levels = []
        self.coarse = None
        self._world = dist_A.world
        self._build(dist_A)
        self._build_sell()

    def _build_sell(self):
        """SELL-64 images for the distributed levels' device-resident parts
        (same policy/measurements as precond/amg.py: >= 500k local rows).
        The DistBackend's spmv dispatches on A_loc, so the conversion is
        transparent to the V-cycle."""
        import os

        if getattr(self.base, "name", "") != "hip" or os.environ.get("AMGCL_NO_SELL"):
            return
        from ..backend.hip import DeviceCSR

        def conv(M):
            if isinstance(M, DeviceCSR) and M.nrows >= 500_000:
                M.build_sell(compact="auto")
            elif isinstance(M, DistMatrix) and isinstance(M.A_loc, DeviceCSR) \
                    and M.A_loc.nrows >= 500_000:
                M.A_loc.build_sell(compact="auto")

        for L in self.levels:
            for name in ("A", "P", "R"):
                M = getattr(L, name, None)  # __slots__: coarsest has no P/R
                if M is not None:
                    conv(M)

    # --- setup ---------------------------------------------------------------
    def _strip_scipy(self, A: DistMatrix):
        """The rank's row strip as (A_loc, A_rem) scipy matrices + ghost ids."""
        loc = A.A_loc_host.to_scipy()
        rem = A.A_rem_host.to_scipy() if A.A_rem_host is not None else None
        return loc, rem

    def _exchange_p_rows(self, A: DistMatrix, P, coarse_beg):
        """Fetch the P rows of A's ghost columns from their owners.

        Every rank packs, for each neighbor, the P rows that neighbor's
        ghosts reference (A.send_idx lists exactly those rows, in the order
        the neighbor's ghost slice expects). Returns P_ghost as a scipy CSR
        (n_ghost x n_coarse_global)."""
        import scipy.sparse as sp

        Pl = P.tocsr()
        packets = {}
        for r, idx in zip(A.send_ranks, A.send_idx):
            rows = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx,
                              dtype=np.int64)
            sub = Pl[rows]
            packets[r] = (sub.indptr, sub.indices + coarse_beg[A.rank], sub.data)
        gathered = [None] * A.world
        self.dist.all_gather_object(gathered, packets, group=self.group)

        n_coarse_glob = int(coarse_beg[-1])
        if A.n_ghost == 0:
            return sp.csr_matrix((0, n_coarse_glob))
        blocks = []
        for r in A.recv_ranks:
            ptr, col, val = gathered[r][A.rank]
            nr = len(ptr) - 1
            blocks.append(sp.csr_matrix((val, col, ptr), shape=(nr, n_coarse_glob)))
        return sp.vstack(blocks, format="csr")

    def _build(self, A: DistMatrix):
        eps = float(self.prm["coarsening"]["eps_strong"])
        relax = self.prm["relax"]["type"]
        damping = float(self.prm["relax"]["damping"])
        coarse_enough = int(self.prm["coarse_enough"])
        max_levels = int(self.prm["max_levels"])

        while True:
            L = _Level()
            L.A = A
            L.n_loc = A.n_loc
            L.f = self.base.vector(A.n_loc)
            L.u = self.base.vector(A.n_loc)
            L.t = self.base.vector(A.n_loc)
            # smoother weights from the full strip row (local + remote)
            loc, rem = self._strip_scipy(A)
            dia = loc.diagonal()
            if relax == "spai0":
                den = np.asarray(loc.multiply(loc).sum(axis=1)).ravel()
                if rem is not None:
                    den += np.asarray(rem.multiply(rem).sum(axis=1)).ravel()
                m = np.divide(dia, den, out=np.zeros_like(dia), where=den != 0)
            elif relax == "damped_jacobi":
                m = np.divide(damping, dia, out=np.zeros_like(dia),
                              where=dia != 0)
            else:
                raise ValueError(f"dist_amg relax '{relax}' not supported")
            L.M = self.base.from_host(m)

            sizes = [None] * A.world
            self.dist.all_gather_object(sizes, A.n_loc, group=self.group)
            n_glob = int(np.sum(sizes))
            small = (n_glob <= int(self.prm["repart_threshold"])
                     or len(self.levels) + 1 >= max_levels
                     or min(sizes) < 50)  # starved strip: stop coarsening
            if small:
                self.levels.append(L)
                self._build_coarse_solver(A, n_glob > coarse_enough)
                break

            if self.prm["coarsening"]["cross_rank"]:
                A = self._step_down_pmis(A, L, eps, sizes)
                eps *= 0.5
                self.levels.append(L)
                continue

            # rank-local aggregation + smoothed prolongation (host engine)
            Ah = A.A_loc_host
            agg = (_core.aggregates_parallel if Ah.nrows > 100_000
                   else _core.aggregates)
            naggr, ids, strong = agg(Ah.nrows, Ah.ptr, Ah.col, Ah.val, eps)
            eps *= 0.5
            if naggr == 0 or naggr >= Ah.nrows:
                self.levels.append(L)
                self._build_coarse_solver(A)
                break
            pp, pc, pv = _core.smoothed_prolongation(
                Ah.nrows, Ah.ptr, Ah.col, Ah.val, strong, ids, naggr, 2.0 / 3.0
            )
            P_host = CSR(Ah.nrows, naggr, pp, pc, pv)
            L.P = self.base.matrix(P_host)
            L.R = self.base.matrix(P_host.transpose())
            self.levels.append(L)

            # distributed Galerkin: Ac = P^T (A_loc P + A_rem P_ghost)
            naggrs = [None] * A.world
            self.dist.all_gather_object(naggrs, naggr, group=self.group)
            coarse_beg = np.concatenate([[0], np.cumsum(naggrs)]).astype(np.int64)
            import scipy.sparse as sp

            Pl = P_host.to_scipy()
            # local columns shifted to the global coarse numbering
            Pg = sp.csr_matrix(
                (Pl.data, Pl.indices + coarse_beg[A.rank], Pl.indptr),
                shape=(Ah.nrows, int(coarse_beg[-1])),
            )
            mid = loc @ Pg
            if rem is not None:
                P_ghost = self._exchange_p_rows(A, Pl, coarse_beg)
                mid = mid + rem @ P_ghost
            Ac = (Pl.T @ mid).tocsr()
            Ac.sort_indices()
            strip = CSR.from_scipy(Ac)
            A = DistMatrix(strip, self.base, self.group)

    def _step_down_pmis(self, A, L, eps, sizes):
        """Cross-rank pmis aggregation + distributed transfer operators
        (parity: mpi/coarsening/pmis.hpp — aggregates cross rank boundaries;
        P/R are rectangular DistMatrix over the coarse partition and the
        V-cycle transfers halo-exchange)."""
        from . import pmis

        ids, S_loc, S_rem = pmis.pmis_aggregates(A, eps, self.dist, self.group)
        coarse_of, naggr_sizes, coarse_begs = pmis.renumber(
            A, ids, self.dist, self.group)
        P = pmis.smoothed_p_strip(A, coarse_of, S_loc, S_rem,
                                  int(coarse_begs[-1]), 2.0 / 3.0,
                                  self.dist, self.group)
        R = pmis.transpose_exchange(A, P, coarse_begs, self.dist, self.group)
        Ac = pmis.galerkin_strip(A, P, coarse_begs, self.dist, self.group)
        L.P = DistMatrix(CSR.from_scipy(P), self.base, self.group,
                         col_sizes=naggr_sizes)
        L.R = DistMatrix(CSR.from_scipy(R), self.base, self.group,
                         col_sizes=sizes)
        return DistMatrix(CSR.from_scipy(Ac), self.base, self.group)

    def _build_coarse_solver(self, A: DistMatrix, as_amg_tail=False):
        """Replicate the global coarse problem on every rank: either a dense
        inverse (global size <= coarse_enough) or a full serial AMG tail that
        continues the hierarchy redundantly (merge-repartition semantics)."""
        import scipy.sparse as sp

        g = int(self.prm["coarse_group_size"])
        self._cg_master = None
        self._cg_group = None
        self._cg_rank = A.rank
        is_master = True
        if g > 1 and A.world > 1:
            my_master = (A.rank // g) * g
            for m0 in range(0, A.world, g):
                ranks = list(range(m0, min(m0 + g, A.world)))
                grp = self.dist.new_group(ranks=ranks)
                if m0 == my_master:
                    self._cg_group = grp
            self._cg_master = my_master
            is_master = A.rank == my_master

        loc, rem = self._strip_scipy(A)
        # re-express the strip with global columns
        cols_g = np.asarray(A.A_loc_host.col, dtype=np.int64) + A.row_beg
        parts = [sp.csr_matrix(
            (A.A_loc_host.val, cols_g, A.A_loc_host.ptr),
            shape=(A.n_loc, A.n_global))]
        if A.A_rem_host is not None:
            gg = np.asarray(A.ghost_global, dtype=np.int64)
            parts.append(sp.csr_matrix(
                (A.A_rem_host.val, gg[np.asarray(A.A_rem_host.col)],
                 A.A_rem_host.ptr), shape=(A.n_loc, A.n_global)))
        strip = parts[0] if len(parts) == 1 else (parts[0] + parts[1])
        gathered = [None] * A.world
        self.dist.all_gather_object(
            gathered, (strip.indptr, strip.indices, strip.data),
            group=self.group)
        if not is_master:
            # slaves hold no coarse system at all (subcommunicator mode)
            self.coarse = None
            self.tail = None
            G_csr = None
        else:
            rows = [sp.csr_matrix((v, c, p), shape=(len(p) - 1, A.n_global))
                    for p, c, v in gathered]
            G = sp.vstack(rows, format="csr")
            G.sort_indices()
            G_csr = CSR.from_scipy(G)
        if not is_master:
            pass
        elif as_amg_tail:
            # replicated serial AMG tail: every rank continues the SAME
            # hierarchy below this level and applies it redundantly
            from ..precond import make_preconditioner

            self.coarse = None
            self.tail = make_preconditioner(
                G_csr,
                {"class": "amg",
                 "coarse_enough": int(self.prm["coarse_enough"]),
                 "npre": int(self.prm["npre"]), "npost": int(self.prm["npost"]),
                 "ncycle": int(self.prm["ncycle"]),
                 "relax": ({"type": "damped_jacobi",
                            "damping": float(self.prm["relax"]["damping"])}
                           if self.prm["relax"]["type"] == "damped_jacobi"
                           else {"type": self.prm["relax"]["type"]})},
                self.base)
        else:
            self.coarse = self.base.coarse_solver(
                G_csr, kind=str(self.prm["direct_solver"]))
            self.tail = None
        self._is_cg_master = is_master
        self._coarse_n = A.n_global
        self._coarse_sizes = [len(p) - 1 for p, _, _ in gathered]
        self._coarse_beg = int(np.sum(self._coarse_sizes[: A.rank]))
        import torch

        dev = getattr(self.base, "device", "cpu")
        pad = max(self._coarse_sizes)
        self._gbuf = torch.zeros(A.world * pad, dtype=torch.float64,
                                 device=dev if self.base.name == "hip" else "cpu")
        self._gpad = pad
        self._gf = self.base.vector(A.n_global)
        self._gu = self.base.vector(A.n_global)

    # --- apply ---------------------------------------------------------------
    def _coarse_solve(self, f, u):
        """All-gather the coarse rhs strips, solve replicated, slice ours."""
        import torch

        if self._world == 1:  # single rank: the strip IS the global problem
            if self.coarse is not None:
                self.coarse(f, u)
            else:
                self.tail.apply(f, u)
            return
        t = self._as_tensor(f)
        pad = self._gpad
        send = torch.zeros(pad, dtype=torch.float64, device=self._gbuf.device)
        send[: t.numel()] = t
        bufs = list(self._gbuf.view(-1, pad))
        self.dist.all_gather(bufs, send, group=self.group)
        gf = self._as_tensor(self._gf)
        off = 0
        for r, sz in enumerate(self._coarse_sizes):
            gf[off : off + sz] = self._gbuf[r * pad : r * pad + sz]
            off += sz
        if self._cg_master is not None:
            # subcommunicator mode: only the group master solves; the group
            # receives the global solution by broadcast (solver_base shape)
            if self._is_cg_master:
                if self.coarse is not None:
                    self.coarse(self._gf, self._gu)
                else:
                    self.tail.apply(self._gf, self._gu)
            self.dist.broadcast(self._as_tensor(self._gu), src=self._cg_master,
                                group=self._cg_group)
        elif self.coarse is not None:
            self.coarse(self._gf, self._gu)
        else:
            self.tail.apply(self._gf, self._gu)  # replicated hierarchy tail
        self._as_tensor(u)[:] = self._as_tensor(self._gu)[
            self._coarse_beg : self._coarse_beg + t.numel()]

    def _as_tensor(self, v):
        import torch

        return torch.from_numpy(v) if isinstance(v, np.ndarray) else v

    def _relax(self, L, rhs, x):
        b = self.backend
        b.residual(rhs, L.A, x, L.t)
        self.base.vmul(1.0, L.M, L.t, 1.0, x)

    def _cycle(self, k):
        L = self.levels[k]
        if k == len(self.levels) - 1:
            self._coarse_solve(L.f, L.u)
            return
        C = self.levels[k + 1]
        b = self.backend
        self.base.clear(L.u)
        for _ in range(int(self.prm["ncycle"])):
            for _ in range(int(self.prm["npre"])):
                self._relax(L, L.f, L.u)
            b.residual(L.f, L.A, L.u, L.t)
            # decoupled transfers are rank-local; cross-rank (pmis) transfers
            # are rectangular DistMatrix and halo-exchange
            tb = b if isinstance(L.R, DistMatrix) else self.base
            tb.spmv(1.0, L.R, L.t, 0.0, C.f)
            self._cycle(k + 1)
            tb = b if isinstance(L.P, DistMatrix) else self.base
            tb.spmv(1.0, L.P, C.u, 1.0, L.u)
            for _ in range(int(self.prm["npost"])):
                self._relax(L, L.f, L.u)

    def apply(self, rhs, x):
        L = self.levels[0]
        self.base.copy(rhs, L.f)
        self._cycle(0)
        self.base.copy(L.u, x)

    def system_matrix(self):
        return self.levels[0].A

    def __str__(self):
        lines = ["DistAMG (decoupled aggregation, coupled Galerkin)"]
        for k, L in enumerate(self.levels):
            lines.append(f"  level {k}: n_loc={L.n_loc}")
        return "\n".join(lines)
