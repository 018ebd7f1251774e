#!/usr/bin/env python3
"""Flagship benchmark (driver contract).

Metric (BASELINE.json): setup+solve time (s) and iterations to rel. 1e-6 on a
synthetic 7-point 3D Poisson system (512^3 default) with a random RHS,
CG + smoothed-aggregation AMG + SPAI0, fp64, at 1/2/4/8 MI355X GPUs.

One "step" = one full setup (host hierarchy assembly) + solve (GPU) cycle.
Strong scaling: the 512^3 problem is partitioned in row blocks across ranks.

Single GPU:  python bench.py [--size 512 --steps 1 --warmup 1]
Multi GPU :  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                 --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run sets up, warms up, times the steps and prints one JSON line.
--dump-outputs DIR additionally writes what the last timed step returned
(x.npy, iters.npy, resid.npy) so two builds can be compared output for
output; the inputs are seeded and identical from run to run.
--full is reserved for secondary measurements (other configurations,
baselines, per-kernel figures); none live in this file today — they are
separate tools under scripts/ — so it currently adds nothing to a plain run.
"""
import argparse
import json
import os
import sys
import time

# Multi-GB setup blocks (SELL images, SpGEMM outputs) must be reusable
# across steps: forbid splitting big cached blocks, otherwise the warm
# steps pay fresh hipMalloc (~28 ms/GB measured, profiles/README r02).
os.environ.setdefault("PYTORCH_ALLOC_CONF", "max_split_size_mb:512")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BASELINE_TOTAL_S = 2.03  # MN4 6144 cores: 0.68 setup + 1.35 solve


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    p.add_argument("--steps", type=int, default=1)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--size", type=int, default=512, help="grid edge n (n^3 unknowns)")
    p.add_argument("--tol", type=float, default=1e-6)
    p.add_argument("--solver", default="cg")
    p.add_argument("--maxiter", type=int, default=300)
    p.add_argument("--backend", default=None, choices=[None, "hip", "cpu"])
    p.add_argument("--precond", default=None, help="override precond JSON")
    p.add_argument("--weak", action="store_true",
                   help="weak scaling: size^3 unknowns PER RANK (domain grows "
                        "along z); default is strong scaling at size^3 total")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's outputs "
                        "(x, iters, resid) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary measurements "
                        "(none at present; a plain run is the headline only)")
    return p.parse_args()


# --dump-outputs keeps x whole up to this many entries (32 MiB of fp64);
# a longer x is reduced to a fixed, seeded sample of this many entries
DUMP_MAX_ENTRIES = 1 << 22


def dump_outputs(path, x, iters, resid):
    import numpy as np

    os.makedirs(path, exist_ok=True)
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size > DUMP_MAX_ENTRIES:
        idx = np.random.default_rng(0).integers(0, x.size, size=DUMP_MAX_ENTRIES)
        idx.sort()
        x = x[idx]
    np.save(os.path.join(path, "x.npy"), x)
    np.save(os.path.join(path, "iters.npy"), np.array([iters], dtype=np.float64))
    np.save(os.path.join(path, "resid.npy"), np.array([resid], dtype=np.float64))


def one_step(args, dist_ctx, want_x=False):
    """Full setup+solve; returns (elapsed_s, setup_s, solve_s, iters, resid,
    true_rel, x) where x is the full solution as the solver returned it (host
    array or device tensor) if want_x, else None."""
    import numpy as np

    import amgcl_amd as am

    if dist_ctx is None:
        backend = args.backend or ("hip" if _has_gpu() else "cpu")
        # problem generation is not part of the measured metric
        # (reference "setup" = hierarchy construction, docs/benchmarks.rst).
        # On the GPU the fixture is generated directly in device memory and
        # the whole setup runs on-device.
        if backend == "hip":
            import torch

            from amgcl_amd.backend.hip_setup import poisson3d_device

            A = poisson3d_device(args.size)
            g = torch.Generator(device="cuda").manual_seed(42)
            b = torch.randn(args.size**3, dtype=torch.float64, device="cuda",
                            generator=g)
        else:
            A, b = am.poisson3d(args.size, rhs="random")
        prm = {
            "precond": json.loads(args.precond) if args.precond else {"class": "amg"},
            "solver": {"type": args.solver, "tol": args.tol, "maxiter": args.maxiter},
        }
        t0 = time.perf_counter()
        solve = am.make_solver(A, prm, backend=backend)
        solve.backend.synchronize()
        t1 = time.perf_counter()
        if os.environ.get("AMGCL_PROFILE"):
            from amgcl_amd.profiler import prof

            print(prof.report(), file=sys.stderr)
            print(solve.P, file=sys.stderr)
        x, iters, resid = solve(b)
        solve.backend.synchronize()
        t2 = time.perf_counter()
        if backend == "hip":
            import math

            be = solve.backend
            r = be.vector(A.nrows)
            be.residual(b, solve.system_matrix(), x, r)
            true_rel = math.sqrt(be.dot(r, r)) / math.sqrt(be.dot(b, b))
        else:
            xh = solve.backend.to_host(x)
            true_rel = float(np.linalg.norm(b - A @ xh) / np.linalg.norm(b))
    else:
        t0, t1, t2, iters, resid, true_rel, x = run_distributed(args, dist_ctx)
    if not want_x:
        x = None
    return t2 - t0, t1 - t0, t2 - t1, iters, resid, true_rel, x


def run_distributed(args, dist_ctx):
    import numpy as np
    import torch.distributed as dist

    import amgcl_amd as am
    from amgcl_amd.parallel import make_dist_solver

    rank, world = dist_ctx
    n = args.size
    # weak mode: fixed size^3 unknowns per rank, domain elongated along z
    # (BASELINE.md weak-scaling table shape: ~const work per core)
    nz = n * world if args.weak else n
    backend_name = args.backend or ("hip" if _has_gpu() else "cpu")
    device_strip = backend_name == "hip" and not os.environ.get(
        "AMGCL_BENCH_HOST_STRIP")
    if device_strip:
        # strip generated directly in device memory (the distributed twin of
        # the 1-GPU fixture path); b moves up once, outside the timed region
        import torch

        from amgcl_amd.backend.hip_setup import poisson3d_device_strip

        ntot = n * n * nz
        row_beg = rank * ntot // world
        row_end = (rank + 1) * ntot // world
        A_strip = poisson3d_device_strip(n, row_beg, row_end, nz=nz)
    elif backend_name == "hip" and not args.weak:
        A_strip, _, row_beg, row_end = am.poisson3d_strip(n, rank, world, rhs=None)
    elif args.weak:
        from amgcl_amd.generators import poisson3d_box_strip

        A_strip, _, row_beg, row_end = poisson3d_box_strip(n, n, nz, rank, world,
                                                           rhs=None)
    else:
        A_strip, _, row_beg, row_end = am.poisson3d_strip(n, rank, world, rhs=None)
    if args.weak:
        rng = np.random.default_rng(42 + rank)
        b = rng.standard_normal(row_end - row_beg)
    else:
        rng = np.random.default_rng(42)
        b = rng.standard_normal(n * n * nz)[row_beg:row_end]
    if backend_name == "hip":
        b = __import__("torch").from_numpy(b).cuda()
    # linear subdomain deflation, the reference's flagship distributed config
    # (MN4 strong scaling uses SDD linear deflation)
    idx = np.arange(row_beg, row_end)
    coords = np.stack(
        [idx % n, (idx // n) % n, idx // (n * n)],
        axis=1,
    ).astype(np.float64)
    pprm = json.loads(args.precond) if args.precond else {"class": "amg"}
    prm = {
        "precond": pprm,
        "solver": {"type": args.solver, "tol": args.tol, "maxiter": args.maxiter},
        "deflation": {"type": "linear", "coords_raw": coords},
    }
    if pprm.get("class") == "dist_amg":
        # one hierarchy over the whole operator already couples the ranks;
        # subdomain deflation is the block-Jacobi path's accelerator
        prm.pop("deflation")
    dist.barrier()
    t0 = time.perf_counter()
    try:
        solve = make_dist_solver(A_strip, prm, backend=backend_name)
    except Exception:
        if not device_strip:
            raise
        # deterministic escape hatch: rebuild from the host strip (the
        # r01-proven path) if the device-resident strip path fails
        import traceback

        traceback.print_exc()
        print(f"[bench rank {rank}] device-strip path failed; "
              "falling back to host strip", file=sys.stderr)
        device_strip = False
        A_strip, _, _, _ = (am.poisson3d_strip(n, rank, world, rhs=None)
                            if not args.weak else
                            __import__("amgcl_amd.generators",
                                       fromlist=["poisson3d_box_strip"])
                            .poisson3d_box_strip(n, n, nz, rank, world, rhs=None))
        dist.barrier()
        t0 = time.perf_counter()
        solve = make_dist_solver(A_strip, prm, backend=backend_name)
    solve.backend.synchronize()
    dist.barrier()
    t1 = time.perf_counter()
    x, iters, resid = solve(b)
    solve.backend.synchronize()
    dist.barrier()
    t2 = time.perf_counter()
    # True residual check, strip-local: every rank computes
    # ||b_strip - A_strip x_full||^2 against its own strip (global columns)
    # and the norms are all-reduced.  This is exactly ||b - A x|| without
    # rebuilding the full operator anywhere (a host 512^3 assembly costs
    # ~2.5 min of untimed wall on a quota-limited box, per run).
    xs = [None] * world
    xh = solve.backend.to_host(x)
    dist.all_gather_object(xs, np.asarray(xh, dtype=np.float64))
    x_full = np.concatenate(xs)
    import torch

    if device_strip:
        xd = torch.from_numpy(x_full).cuda()
        r = torch.empty(A_strip.nrows, dtype=torch.float64, device="cuda")
        solve.backend.base.spmv(1.0, A_strip, xd, 0.0, r)
        r = b - r
        nums = torch.stack([r @ r, b @ b]).cpu()
    else:
        bh = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b, dtype=np.float64)
        r = bh - A_strip @ x_full
        nums = torch.tensor([float(r @ r), float(bh @ bh)], dtype=torch.float64)
    if dist.get_backend() == "nccl":
        nums = nums.cuda()  # NCCL collectives need device tensors
    dist.all_reduce(nums)
    true_rel = float((nums[0] / nums[1]).sqrt())
    return t0, t1, t2, iters, resid, true_rel, x_full


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist_ctx = None
    if world > 1:
        import torch
        import torch.distributed as dist

        rank = int(os.environ["RANK"])
        local_rank = int(os.environ.get("LOCAL_RANK", rank))
        if _has_gpu():
            # modulo allows oversubscribed single-GPU testing; in production
            # one rank per GPU (local_rank < device_count)
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
            dist.init_process_group("nccl")
        else:
            dist.init_process_group("gloo")
        dist_ctx = (rank, world)

    rank = dist_ctx[0] if dist_ctx else 0

    for _ in range(args.warmup):
        one_step(args, dist_ctx)

    if dist_ctx:
        import torch.distributed as dist

        dist.barrier()
    times, setups, solves, iters_l, resid, true_rel = [], [], [], [], 0.0, 0.0
    t_start = time.perf_counter()
    x = None
    for i in range(args.steps):
        el, setup_s, solve_s, iters, resid, true_rel, x = one_step(
            args, dist_ctx,
            want_x=bool(args.dump_outputs) and i == args.steps - 1)
        times.append(el)
        setups.append(setup_s)
        solves.append(solve_s)
        iters_l.append(iters)
    total = time.perf_counter() - t_start

    if dist_ctx:
        import torch
        import torch.distributed as dist

        t = torch.tensor([total], dtype=torch.float64,
                         device="cuda" if _has_gpu() else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        total = float(t.item())

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, x, iters_l[-1], resid)

    if rank == 0:
        value = total / args.steps
        weak = bool(args.weak and world > 1)
        metric = (f"setup+solve time (s) & iterations to 1e-6, 3D Poisson "
                  f"{args.size}^3" + ("/GPU (weak)" if weak else ""))
        out = {
            "metric": metric,
            "value": value,
            "unit": "s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": value * 1000.0,
            "higher_is_better": False,
            "scaling": "weak" if weak else "strong",
            "vs_baseline": None if weak else value / BASELINE_TOTAL_S,
            "dtype": "fp64",
            "data": "synthetic 7-pt Poisson, random RHS",
            "config": {
                "model": f"3D Poisson {args.size}^3 (7-point stencil)",
                "unknowns": args.size**3 * (world if weak else 1),
                "solver": args.solver,
                "precond": "smoothed_aggregation AMG + SPAI0",
                "tol": args.tol,
                "iters": iters_l[-1],
                "setup_s": setups[-1],
                "solve_s": solves[-1],
                "final_rel_resid": resid,
                "true_rel_resid": true_rel,
                "parallelism": f"row-block dd x{world}" if world > 1 else "single GPU",
            },
        }
        print(json.dumps(out))

    if dist_ctx:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
