"""The driver contract: bench.py must run the distributed path end-to-end
(torch.distributed env vars, one process per rank) and emit one JSON line
with the agreed fields. Runs on CPU over gloo — the same code path the
round-end 8-GPU scale run exercises over RCCL."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp


def _run_bench(rank, world, port, argv, results):
    os.environ.update(
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
        LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
    )
    sys.argv = ["bench.py"] + argv
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    buf = io.StringIO()
    real = sys.stdout
    sys.stdout = buf
    try:
        bench.main()
    finally:
        sys.stdout = real
    results[rank] = buf.getvalue()


@pytest.mark.parametrize("world,extra", [
    (4, []),
    (2, ["--precond", '{"class": "dist_amg", "coarse_enough": 200,'
                      ' "repart_threshold": 400}']),
    (2, ["--weak"]),
])
def test_bench_distributed_contract(world, extra):
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        argv = ["--size", "24", "--steps", "2", "--warmup", "1",
                "--backend", "cpu"] + extra
        procs = [ctx.Process(target=_run_bench,
                             args=(r, world, 29391 + world, argv, results))
                 for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
        for p in procs:
            assert p.exitcode == 0
        out = dict(results)
    # only rank 0 prints; exactly one JSON line
    lines = [ln for ln in out[0].strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    for r in range(1, world):
        assert out[r].strip() == ""
    d = json.loads(lines[0])
    weak = "--weak" in extra
    assert d["n_gpus"] == world
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["scaling"] == ("weak" if weak else "strong")
    assert d["dtype"] == "fp64"
    assert d["higher_is_better"] is False
    assert d["unit"] == "s"
    assert abs(d["ms_per_step"] - d["value"] * 1000) < 1e-9
    if weak:
        assert d["vs_baseline"] is None
        assert d["config"]["unknowns"] == 24 ** 3 * world
    else:
        assert abs(d["vs_baseline"] - d["value"] / 2.03) < 1e-12
        assert d["config"]["unknowns"] == 24 ** 3
    assert d["config"]["true_rel_resid"] < 1e-6
    assert "Poisson 24^3" in d["metric"]


def test_bench_single_process_contract():
    import subprocess

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run(
        [sys.executable, "bench.py", "--size", "20", "--steps", "1",
         "--warmup", "1", "--backend", "cpu"],
        capture_output=True, text=True, timeout=300,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1
    assert d["config"]["true_rel_resid"] < 1e-6


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes what the last timed step returned; the inputs
    are seeded, so the dumped x must solve the same system rebuilt here.
    --full is accepted alongside and keeps the single result line."""
    import subprocess

    import amgcl_amd as am

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out_dir = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, "bench.py", "--size", "16", "--steps", "2",
         "--warmup", "0", "--backend", "cpu", "--full",
         "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=300,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 0
    assert abs(d["ms_per_step"] - d["value"] * 1000) < 1e-9
    assert sorted(p.name for p in out_dir.iterdir()) == [
        "iters.npy", "resid.npy", "x.npy"]
    x = np.load(out_dir / "x.npy")
    iters = np.load(out_dir / "iters.npy")
    resid = np.load(out_dir / "resid.npy")
    assert x.dtype == np.float64 and x.shape == (16 ** 3,)
    assert iters.dtype == np.float64 and resid.dtype == np.float64
    assert int(iters[0]) == d["config"]["iters"]
    assert float(resid[0]) == d["config"]["final_rel_resid"]
    A, b = am.poisson3d(16, rhs="random")
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) < 1e-6


def test_bench_dump_sample_is_fixed(tmp_path):
    """An output longer than the cap is reduced to a fixed, seeded sample:
    same entries on every call, in increasing index order."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    n = bench.DUMP_MAX_ENTRIES + 12345
    x = np.arange(n, dtype=np.float64)
    bench.dump_outputs(str(tmp_path / "a"), x, 7, 1e-7)
    bench.dump_outputs(str(tmp_path / "b"), x, 7, 1e-7)
    a = np.load(tmp_path / "a" / "x.npy")
    b = np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (bench.DUMP_MAX_ENTRIES,) and a.dtype == np.float64
    assert np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < n
    assert a.nbytes <= 64 * 2 ** 20
