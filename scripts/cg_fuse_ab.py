"""Fused against unfused CG solve on ONE hierarchy (usage: cg_fuse_ab.py [n]).

The setup is run once; the native driver is then created on that hierarchy
with and without AMGCL_NO_FUSE=1 (read at driver creation), twice each, and
the flagship right-hand side is solved.  Holding the setup fixed takes its
run-to-run states (profiles/README.md) out of the comparison, so what is left
is the fused kernels against the kernels they replace.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import amgcl_amd as am  # noqa: E402
from amgcl_amd.backend.hip_setup import poisson3d_device  # noqa: E402
from amgcl_amd.backend.native import try_native  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
A = poisson3d_device(n)
g = torch.Generator(device="cuda").manual_seed(42)
b = torch.randn(n**3, dtype=torch.float64, device="cuda", generator=g)
prm = {"precond": {"class": "amg"},
       "solver": {"type": "cg", "tol": 1e-6, "maxiter": 300}}
os.environ.pop("AMGCL_NO_FUSE", None)
solve = am.make_solver(A, prm, backend="hip")
runs = {}
for tag, nofuse in (("fused 1", False), ("unfused 1", True), ("unfused 2", True),
                    ("fused 2", False)):
    if nofuse:
        os.environ["AMGCL_NO_FUSE"] = "1"
    else:
        os.environ.pop("AMGCL_NO_FUSE", None)
    solve._native = try_native(solve)
    x, iters, resid = solve(b)
    torch.cuda.synchronize()
    runs[tag] = x.clone()
    print(f"{tag}: {iters} iterations, resid {resid!r}", flush=True)
xmax = float(runs["unfused 1"].abs().max())
for a, c in (("unfused 1", "unfused 2"), ("fused 1", "fused 2"),
             ("fused 1", "unfused 1"), ("fused 2", "unfused 2")):
    d = float((runs[a] - runs[c]).abs().max())
    print(f"max|x({a}) - x({c})| = {d:.3e}  (max|x| = {xmax:.3f})", flush=True)
