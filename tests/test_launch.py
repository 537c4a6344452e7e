"""The single-node launcher (oneflow_spmm/launch.py, the environment contract of the reference's
python/oneflow/distributed/launch.py:103-140) and bench.py's use of it: `--gpus N` without a
launcher spawns N ranks, and a rank count that differs from --gpus is an error.  CPU only
(gloo), plus one GPU rehearsal of the multi-rank bench path."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "of-spmm_amd"))

from oneflow_spmm import launch  # noqa: E402

RANK_SCRIPT = textwrap.dedent("""
    import os, sys
    import torch, torch.distributed as dist
    dist.init_process_group("gloo")   # env:// rendezvous from the launcher's variables
    r, w = dist.get_rank(), dist.get_world_size()
    assert r == int(os.environ["RANK"]) == int(os.environ["LOCAL_RANK"])
    t = torch.tensor([r + 1])
    dist.all_reduce(t)
    with open(os.path.join(sys.argv[1], f"rank{r}"), "w") as f:
        f.write(f"{w} {int(t)} {sys.argv[2]}")
    dist.destroy_process_group()
""")


def test_spawn_runs_every_rank_with_the_env_contract(tmp_path):
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT)
    rc = launch.spawn_local_ranks(3, [str(script), str(tmp_path), "arg"], timeout=120)
    assert rc == 0
    for r in range(3):
        assert (tmp_path / f"rank{r}").read_text() == "3 6 arg"  # world 3, sum of 1+2+3


def test_spawn_reports_the_failing_rank_and_stops_the_rest(tmp_path):
    script = tmp_path / "fail.py"
    script.write_text(textwrap.dedent("""
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(3)
        time.sleep(120)
    """))
    import time
    t0 = time.monotonic()
    rc = launch.spawn_local_ranks(2, [str(script)], timeout=200)
    assert rc == 3
    assert time.monotonic() - t0 < 60  # rank 0 was terminated, not waited for


def test_rank_env():
    env = launch.rank_env({"X": "1"}, 4, 2, "127.0.0.1", 1234)
    assert env["X"] == "1" and env["WORLD_SIZE"] == "4" and env["RANK"] == "2"
    assert env["LOCAL_RANK"] == "2" and env["MASTER_ADDR"] == "127.0.0.1"
    assert env["MASTER_PORT"] == "1234"


def _bench(args, env_extra, drop=()):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env,
                          capture_output=True, text=True, timeout=300)


def test_bench_refuses_a_rank_count_other_than_gpus():
    p = _bench(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2, p.stderr[-2000:]
    assert "WORLD_SIZE=1" in p.stderr
    assert p.stdout == ""  # no JSON line for a run that did not happen


def test_bench_spawns_its_ranks_without_a_launcher():
    """No WORLD_SIZE: the parent starts --gpus ranks (before any GPU call) and exits with their
    status; on this CPU-only container every rank then fails at the GPU, so the status is
    non-zero and comes from the ranks, not from a silent one-rank run."""
    p = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {},
               drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"))
    assert "spawning 2 local ranks" in p.stderr
    assert p.returncode != 0
    assert '"n_gpus": 1' not in p.stdout


@pytest.mark.gpu
def test_bench_multi_rank_rehearsal_on_one_gpu():
    """The whole N>1 bench path (self-spawn, process group, RowSplitSpmm bind + tune over every
    exchange candidate, barrier-bracketed timing, max-over-ranks reduction, one JSON line from
    rank 0) on the GPUs this box has, with gloo moving the bytes: a rehearsal of the driver's
    multi-GPU run, flagged as such in the line."""
    import json
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = _bench(["--gpus", "2", "--backend", "gloo", "--config", "plaw1m", "--steps", "2",
                "--warmup", "1", "--full"], {},
               drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"))
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["extra"]["ranks_seen"] == 2 and line["value"] > 0
    assert line["config"]["parallelism"].startswith("REHEARSAL")
    assert len(line["extra"]["allgather_tune_ms"]) >= 5



def _bench_line(p):
    import json
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_SPAWN_ENV_DROP = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")


def test_bench_eight_rank_rehearsal_pinned_grid2x4_s2():
    """the driver's 8-GPU bench path rehearsed with 8 ranks on the host
    (self-spawn, gloo, RowSplitSpmm over host tensors with the kCPU kernel): --exchange
    grid2x4/s2 is accepted and runs, every rank joins, one JSON line with the memory record."""
    p = _bench(["--gpus", "8", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--exchange", "grid2x4/s2", "--steps", "1", "--warmup", "0"],
               {"OMP_NUM_THREADS": "1"}, drop=_SPAWN_ENV_DROP)
    line = _bench_line(p)
    assert line["n_gpus"] == 8 and line["extra"]["ranks_seen"] == 8
    assert line["extra"]["exchange"] == "grid2x4/s2"
    assert line["config"]["parallelism"].startswith("REHEARSAL")
    assert line["extra"]["memory_gb"]["host_rss_peak_sum"] > 0
    assert line["value"] > 0


def test_bench_eight_rank_tune_is_ordered_and_bounded():
    """tune() at 8 ranks: the north star's plain row split + all-gather ("torch/p1" under gloo,
    "rccl/p1" on the node) is measured first and always, every candidate is reported with its
    model time, and a zero budget stops after that first measurement (the rest 'skipped:
    budget'); the line reports the all-gather's number beside the winner."""
    p = _bench(["--gpus", "8", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--steps", "1", "--warmup", "0", "--tune-budget", "0", "--full"],
               {"OMP_NUM_THREADS": "1"}, drop=_SPAWN_ENV_DROP)
    line = _bench_line(p)
    cands = line["extra"]["tune_candidates"]
    assert len(cands) >= 12  # 3 all-gather depths (gloo: one kind), 3 halo, 6 grids
    assert all("predicted_ms" in c for c in cands.values())
    order = list(cands)  # the measurement order: the north star first, every 1-D before grids
    assert order[0] == "torch/p1"
    is_2d = [k.startswith(("grid", "nsplit")) for k in order]
    assert is_2d == sorted(is_2d) and any(is_2d)
    measured = [k for k, c in cands.items() if c["status"] == "measured"]
    assert measured == ["torch/p1"]
    assert all(c["status"] == "skipped: budget" for k, c in cands.items() if k != "torch/p1")
    assert line["extra"]["exchange"] == "allgather"
    ag = line["extra"]["rowsplit_allgather_p1"]
    assert ag["ms"] > 0 and ag["gflops"] > 0
    # every rank logged its phases
    for r in range(8):
        assert f"[rank {r}/8]" in p.stderr and "phase: tune: torch/p1" in p.stderr


def test_bench_eight_rank_value_is_the_rowsplit_even_when_a_grid_is_faster():
    """at 8 ranks the line's value and label come from the 1-D row split the
    north star names (all-gather or halo), even when a 2-D grid measured faster (injected: the
    tests-only OFX_TUNE_TEST_SCALE divides every grid's measured time by 10^4).  The label is
    built from the kept exchange, the grid is reported under extra.grid_best, and every rank
    joined the exchange's communicator."""
    p = _bench(["--gpus", "8", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--steps", "2", "--warmup", "1", "--tune-budget", "600", "--full"],
               {"OMP_NUM_THREADS": "1", "OFX_TUNE_TEST_SCALE": "grid:1e-4,nsplit:1e-4"},
               drop=_SPAWN_ENV_DROP)
    line = _bench_line(p)
    ex = line["extra"]
    cands = ex["tune_candidates"]
    kept = ex["exchange"]
    assert kept in ("allgather", "halo") and ex["exchange_is_rowsplit"]
    # the grid measured fastest, and was not kept
    g = ex["grid_best"]
    assert g is not None and g["exchange"].startswith(("grid", "nsplit"))
    tune = {k: v for k, v in ex["allgather_tune_ms"].items() if v is not None}
    assert min(tune, key=tune.get) == g["exchange"]
    kept_name = min((k for k in tune if not k.startswith(("grid", "nsplit"))), key=tune.get)
    assert cands[kept_name]["status"] == "measured"
    # the label names what ran
    par = line["config"]["parallelism"]
    assert par.startswith("REHEARSAL") and "1-D row split x8" in par
    if kept == "halo":
        assert "halo rows only" in par and kept_name.startswith("halo")
    else:
        assert "all-gather" in par and kept_name.startswith("torch/p")
        depth = int(kept_name.split("/p")[1])
        assert ex["pipeline_blocks"] == depth
        assert (f"{depth} column blocks in sequence" in par) == (depth > 1)  # gloo: no side stream
    assert "grid" not in par
    # value = the whole job's FLOPs over the timed steps of that exchange
    c = line["config"]
    assert abs(line["value"] - 2 * c["nnz"] * c["n"] / (line["ms_per_step"] * 1e-3) / 1e9) \
        <= 1e-3 * line["value"] + 0.02
    assert ex["ranks_seen"] == ex["exchange_comm_ranks"] == line["n_gpus"] == 8
    assert ex["rccl_comm_ranks"] is None  # gloo rehearsal: no RCCL communicator

def test_bench_rebuilds_on_torch_distributed_when_every_native_exchange_fails():
    """A tune whose every native-RCCL candidate failed (the same on every rank: tune's times are
    max-reduced) does not end the run: the exchange is rebuilt on torch.distributed's group and
    tuned again, and the line says so (extra.comm_fallback).  Injected with the tests-only
    '--stall-test 0:native-tune' on the 2-rank gloo rehearsal."""
    p = _bench(["--gpus", "2", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--steps", "2", "--warmup", "1", "--stall-test", "0:native-tune"],
               {"OMP_NUM_THREADS": "1"}, drop=_SPAWN_ENV_DROP)
    line = _bench_line(p)
    ex = line["extra"]
    assert ex["comm_fallback"] and "every exchange failed" in ex["comm_fallback"]
    assert "rebuilding the exchange on torch.distributed" in p.stderr + p.stdout
    assert ex["exchange_is_rowsplit"] and ex["allgather_schedule"] == "torch"
    assert ex["ranks_seen"] == ex["exchange_comm_ranks"] == 2
    assert line["value"] > 0


def test_bench_stalled_rank_names_its_phase_and_fails():
    """A rank stalled in a phase past its limit (injected: rank 1 sleeps in its first tune
    candidate) prints the phase, exits 75, and the launcher ends the run non-zero instead of
    hanging."""
    import time
    t0 = time.monotonic()
    p = _bench(["--gpus", "2", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--steps", "1", "--warmup", "0", "--phase-timeout-scale", "0.05"],
               {"OMP_NUM_THREADS": "1", "OFX_BENCH_STALL": "1:tune"}, drop=_SPAWN_ENV_DROP)
    assert p.returncode != 0
    # rank 1 sleeps; rank 0 waits for it inside the same candidate's collective, so either
    # watchdog may fire first (the launcher then stops the other): the phase is named either way
    assert "STALLED: phase 'tune: torch/p1'" in p.stderr, p.stderr[-3000:]
    assert p.stdout == ""
    assert time.monotonic() - t0 < 120


def test_bench_spawn_deadline_ends_a_hung_run():
    """The launcher's own deadline (--deadline) ends a run whose ranks never finish, with
    timeout(1)'s status 124, whatever the phase limits."""
    import time
    t0 = time.monotonic()
    p = _bench(["--gpus", "2", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--steps", "1", "--warmup", "0", "--deadline", "15", "--phase-timeout-scale",
                "1000"], {"OMP_NUM_THREADS": "1", "OFX_BENCH_STALL": "0:inputs"},
               drop=_SPAWN_ENV_DROP)
    assert p.returncode == 124, p.stderr[-3000:]
    assert time.monotonic() - t0 < 90


def test_bench_eight_ranks_refuses_a_short_launch():
    p = _bench(["--gpus", "8", "--device", "cpu", "--backend", "gloo"],
               {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2 and "WORLD_SIZE=4" in p.stderr and p.stdout == ""


def test_bench_exchange_that_never_completes_is_named_and_fails():
    """a rank whose exchange of B was issued but never completes (injected:
    rank 1 never joins its first all-gather, so rank 0's is stuck after its enqueue) does not hang
    until a phase limit: its exchange deadline fires, the communicator is aborted, the rank names
    the phase and the exchange and exits 76; the launcher ends the run with that status."""
    import time
    t0 = time.monotonic()
    p = _bench(["--gpus", "2", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                "--steps", "1", "--warmup", "0", "--exchange-deadline", "3"],
               {"OMP_NUM_THREADS": "1", "OFX_BENCH_STALL": "1:exchange"}, drop=_SPAWN_ENV_DROP)
    assert p.returncode == 76, p.stderr[-3000:]
    assert "[rank 0/2] EXCHANGE STALLED in phase 'tune: torch/p1'" in p.stderr, p.stderr[-3000:]
    assert "all-gather of B" in p.stderr and "not complete after 3.0 s" in p.stderr
    assert p.stdout == ""
    assert time.monotonic() - t0 < 90


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ofx_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dump_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path):
    """--dump-outputs: an output past the cap is cut to a fixed, seeded, sorted sample of its rows
    (the rows kept are written beside it), float32 on disk (float64 for f64), at most 64 MB in
    all; a small output is written whole."""
    import numpy as np
    import torch
    bench = _load_bench()
    rows, n = 70_000, 128  # 36 MB of fp32: past the cap
    out = torch.arange(rows * n, dtype=torch.float32).reshape(rows, n)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, 0, 1)
    a, ra = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "a" / "out_rows.npy")
    assert sorted(os.listdir(tmp_path / "a")) == ["out.npy", "out_rows.npy"]
    assert a.dtype == np.float32 and ra.dtype == np.float64
    assert a.shape == (bench.DUMP_BYTES // (n * 8), n) and ra.shape == (a.shape[0],)
    assert _dump_bytes(tmp_path / "a") <= 64 << 20
    idx = ra.astype(np.int64)
    assert (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < rows  # sorted, no row twice
    assert np.array_equal(a, out.numpy()[idx])
    assert np.array_equal(a, np.load(tmp_path / "b" / "out.npy"))
    assert np.array_equal(ra, np.load(tmp_path / "b" / "out_rows.npy"))
    # per rank at N>1: its own file, its share of the cap; f64 stays f64, bf16 widens to f32
    bench.dump_outputs(str(tmp_path / "c"), out.double(), 1, 2)
    c = np.load(tmp_path / "c" / "out_rank1.npy")
    assert c.dtype == np.float64 and c.shape == (bench.DUMP_BYTES // 2 // (n * 8), n)
    small = torch.arange(24, dtype=torch.float32).reshape(6, 4).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "d"), small, 0, 1)
    s = np.load(tmp_path / "d" / "out.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "out_rows.npy"), np.arange(6.0))


_FULL_ONLY_KEYS = ("kernel_ms_events_separate_run", "kernel_ms_cold_median", "static_csr_ms_per_step",
                   "allgather_ms_max", "spmm_ms_max", "spmm_phase_gflops_aggregate")


def test_bench_plain_two_rank_run_is_lean_and_its_dump_repeats(tmp_path):
    """A plain N>1 run measures no 2-D grid and no phase on its own (those keys come with --full)
    and still reports the line's figures; --dump-outputs writes every rank's rows of the last
    timed step, float32, bit-identical between two runs with different step counts."""
    import numpy as np
    lines = []
    for d, steps in (("a", "2"), ("b", "3")):
        p = _bench(["--gpus", "2", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
                    "--steps", steps, "--warmup", "1", "--dump-outputs", str(tmp_path / d)],
                   {"OMP_NUM_THREADS": "1"}, drop=_SPAWN_ENV_DROP)
        lines.append(_bench_line(p))
    line = lines[0]
    assert line["steps"] == 2 and lines[1]["steps"] == 3
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert abs(line["value"] - 2 * 200_000 * 32 / (line["ms_per_step"] * 1e-3) / 1e9) \
        <= 1e-3 * line["value"] + 0.02
    ex = line["extra"]
    assert not any(k in ex for k in _FULL_ONLY_KEYS) and "cpu_baseline" not in line
    assert ex["tune_candidates"] and ex["grid_best"] is None
    assert not any(k.startswith(("grid", "nsplit")) for k in ex["tune_candidates"])
    assert ex["exchange_is_rowsplit"] and ex["ranks_seen"] == 2
    assert sorted(os.listdir(tmp_path / "a")) == ["out_rank0.npy", "out_rank0_rows.npy",
                                                  "out_rank1.npy", "out_rank1_rows.npy"]
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b), f
        if not f.endswith("_rows.npy"):
            assert a.dtype == np.float32 and a.shape == (10_000, 32)  # tiny: m = 20000 over 2 ranks
            assert np.isfinite(a).all() and np.abs(a).sum() > 0


def test_bench_plain_one_rank_line_has_no_extras():
    """A plain N=1 run (here on host tensors) prints the line's figures with an empty `extra` and no
    cpu_baseline; with --full both are there."""
    args = ["--gpus", "1", "--backend", "gloo", "--device", "cpu", "--config", "tiny",
            "--steps", "2", "--warmup", "1"]
    line = _bench_line(_bench(args, {"OMP_NUM_THREADS": "1"}, drop=_SPAWN_ENV_DROP))
    assert line["extra"] == {} and "cpu_baseline" not in line
    assert line["steps"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    full = _bench_line(_bench([*args, "--full"], {"OMP_NUM_THREADS": "1"}, drop=_SPAWN_ENV_DROP))
    assert full["extra"]["kernel_ms_events_separate_run"] > 0
    assert full["cpu_baseline"]["bitexact_vs_gpu"] is True
