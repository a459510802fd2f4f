"""bench.py end to end on a GPU, through its own launcher: `python bench.py --gpus 2` (the driver's command) with the
gloo development backend -- two ranks sharing GPU 0, the engine's shared-memory transport between them (RCCL refuses two
ranks on one device and is reported as skipped) -- and the one-rank N > 1 path with both transports in one line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--full: these tests read the roofline object and the extras, which a plain run leaves out)
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "4", "--min-seconds", "0", "--full",
         "--no-cpu-baseline", "--no-extra"]


def run(extra, env, rc=0):
    e = dict(os.environ, **env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    p = subprocess.run(BENCH + extra, env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == rc, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_gpus2_self_launch_gloo(gpu):
    d = run(["--gpus", "2"], {"MUSE_BENCH_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["sims_per_step_total"] == 512
    assert d["transport"] == "shm"
    shm, rccl = d["transports"]["shm"], d["transports"]["rccl"]
    assert shm["collective"] == "shm-capi" and shm["ranks_seen"] == 2
    assert "skipped" in rccl
    assert d["value"] > 0 and abs(d["value"] - 512 / (1e-3 * d["ms_per_step"])) < 1e-6 * d["value"]


def test_bench_gpus8_self_launch_gloo(gpu):
    """The driver's 8-GPU command, as far as one GPU can take it: `python bench.py --gpus 8` starts eight ranks (here all on
    GPU 0, collectives over gloo), the shared-memory communicator counts eight processes, the 512 simulations of a step
    are dealt 8 x 64, every launch carries 8 independent maps, and RCCL -- which refuses several ranks on one device --
    is reported as skipped without costing the line or the exit status."""
    # (the driver's command carries the extras: `--no-extra` of BENCH is dropped here; --small: the extras at sizes eight processes can
    #  share ONE GPU with -- 8 x 17 persistent workgroups of the sharded loop must all be resident at once)
    e = dict(os.environ, MUSE_BENCH_BACKEND="gloo", MUSE_SHARED_GPU_RANKS="16")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    p = subprocess.run([a for a in BENCH if a != "--no-extra"] + ["--gpus", "8", "--small"], env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and d["config"]["sims_per_step_total"] == 512
    assert "(64 on this rank)" in d["config"]["workload"]
    assert d["transport"] == "shm"
    shm, rccl = d["transports"]["shm"], d["transports"]["rccl"]
    assert shm["collective"] == "shm-capi" and shm["ranks_seen"] == 8
    assert shm["pipelining"] == "maps_per_launch=8"
    assert "skipped" in rccl
    assert "independent" in d["config"]["scaling_note"].lower()
    assert d["value"] > 0 and abs(d["value"] - 512 / (1e-3 * d["ms_per_step"])) < 1e-6 * d["value"]
    # round 6: the N > 1 line also carries the DEPENDENT path over these eight ranks -- muse_run_sharded, which loop ran, the boards'
    # hand-shake, the trajectory bit-compared with rank 0's unsharded muse_run on every rank -- and configs[3] / configs[4] sharded,
    # as flat scalars of `config` (what the driver's record keeps)
    c, sh = d["config"], d["sharded"]
    assert c["sharded_bit_equal"] is True and c["sharded_ranks_seen"] == 8, c
    # (EIGHT processes on ONE GPU: the hardware scheduler time-slices their queues in milliseconds -- the hand-shake kernels of the eight
    #  ranks still meet within its 50-ms bound, 10-20 ms measured, but the persistent loop's workgroups of eight processes are never
    #  all running at once, its bounded waits expire and every rank falls back to the host-driven loop together: "none" is the honest
    #  answer here, and the trajectory is the same bits.  Four processes do run side by side: the test below.)
    assert c["handshake_device"] in (0, 1) and c["handshake_host"] in (0, 1) and c["sharded_loop_ran"] in ("device", "host", "none"), c
    assert c["sharded_muse_iter_us"] > 0 and c["sharded_muse_iter_host_board_us"] > 0 and c["sharded_muse_iter_host_loop_us"] > 0
    assert sh["muse_run"]["runs"]["host_loop"]["loop_ran"] == "none"
    assert c["cfg4_fd_H_sharded_ms"] > 0 and c["cfg4_fd_H_sharded_ok"] is True and c["cfg5_smooth_1e5_sharded_ms"] > 0 and c["cfg5_smooth_1e5_sharded_ok"] is True
    assert sh["cfg4_fd_H"]["units_per_rank"] == 32 and sh["cfg5_smooth_1e5"]["sims_per_rank"] == 4


def test_bench_gpus4_sharded_extras_run_the_persistent_loop(gpu):
    """`python bench.py --gpus 4` (four gloo ranks on ONE GPU, which the hardware runs side by side): the N > 1 line's extras -- the
    boards' set-up hand-shake passes for both kinds of board with every rank seeing all four, muse_run_sharded runs as ONE persistent
    launch per rank through the boards in device memory (and through the host's board, and host-driven, when forced), every rank's
    trajectory equals rank 0's unsharded muse_run bit for bit."""
    e = dict(os.environ, MUSE_BENCH_BACKEND="gloo", MUSE_SHARED_GPU_RANKS="8")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    p = subprocess.run([a for a in BENCH if a != "--no-extra"] + ["--gpus", "4", "--small"], env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    c, sh = d["config"], d["sharded"]
    assert d["n_gpus"] == 4 and c["sharded_bit_equal"] is True and c["sharded_ranks_seen"] == 4, c
    assert c["handshake_device"] == 1 and c["handshake_host"] == 1 and c["sharded_board"] == "device" and c["sharded_loop_ran"] == "device", c
    assert 0 < c["handshake_device_wait_us"] < 50e3 and 0 < c["handshake_host_wait_us"] < 50e3, c
    assert [sh["muse_run"]["runs"][k]["loop_ran"] for k in ("default", "host_board", "host_loop")] == ["device", "host", "none"]
    assert sh["muse_run"]["handshake"]["device_seen"] == 15 and sh["muse_run"]["handshake"]["host_seen"] == 15
    assert c["cfg4_fd_H_sharded_ok"] is True and c["cfg5_smooth_1e5_sharded_ok"] is True


def test_bench_under_torch_distributed_run(gpu):
    """The driver's N > 1 command verbatim -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` (bench.py then does NOT start ranks itself: it reads RANK / LOCAL_RANK / WORLD_SIZE) -- with
    two gloo ranks on this one GPU: rank 0 prints ONE JSON line, with the N > 1 extras as flat scalars of `config`."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    e = dict(os.environ, MUSE_BENCH_BACKEND="gloo", MUSE_SHARED_GPU_RANKS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "10", "--warmup", "2", "--min-seconds", "0", "--full", "--small"]
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["transport"] == "shm" and d["transports"]["shm"]["ranks_seen"] == 2
    assert "cpu_baseline" not in d            # (rank 0 at N = 1 only)
    c = d["config"]
    assert c["sharded_bit_equal"] is True and c["sharded_ranks_seen"] == 2 and c["sharded_loop_ran"] == "device", c
    assert c["handshake_device"] == 1 and c["handshake_host"] == 1 and c["cfg4_fd_H_sharded_ok"] is True and c["cfg5_smooth_1e5_sharded_ok"] is True


def test_bench_forced_dist_reports_both_transports(gpu):
    d = run(["--nsims", "64"], {"MUSE_BENCH_FORCE_DIST": "1"})
    assert d["n_gpus"] == 1 and set(d["transports"]) == {"shm", "rccl"}
    for t in ("shm", "rccl"):
        m = d["transports"][t]
        assert m["collective"] == f"{t}-capi" and m["ranks_seen"] == 1, m
    assert d["transport"] in ("shm", "rccl") and d["value"] == max(m["value"] for m in d["transports"].values())


def test_bench_default_line_is_the_single_gpu_workload(gpu):
    d = run([], {})
    assert d["n_gpus"] == 1 and "transports" not in d and d["config"]["element_split"] == 1
    assert d["roofline"]["placement"] == "resident" and d["dtype"] == "f64"


def test_bench_watchdog_reports_without_a_transport_that_hangs(gpu):
    """A second transport that does not finish in time (here: a deadline of a millisecond) must not cost the line: the ranks
    report what the first transport measured and mark the other one -- and leave with a NON-ZERO status (3): a collective
    hung with GPU work in flight, which a launcher or CI must not take for a clean run."""
    d = run(["--nsims", "64"], {"MUSE_BENCH_FORCE_DIST": "1", "MUSE_BENCH_TRANSPORT_DEADLINE_S": "0.001"}, rc=3)
    assert d["transport_failed"] == "rccl"
    assert d["transport"] == "shm" and "watchdog" in d["transports"]["rccl"]["skipped"]
    assert d["transports"]["shm"]["ranks_seen"] == 1 and d["value"] == d["transports"]["shm"]["value"]


def test_bench_gpus8_shards_the_workloads_baseline_puts_on_8_gpus(gpu):
    """configs[3] (get_H! by finite differences, 512 sims x 4 theta) and configs[4] (the stencil model, N = 10^5, 8 theta, 1024
    sims) as `--workload` choices of the driver's 8-GPU command: eight gloo ranks on one GPU, the flattened (sim, column) list in
    eight blocks of 256 units / the 1024 sims in eight blocks of 128, the shared-memory communicator counting eight processes."""
    # (MUSE_SHARED_GPU_RANKS: the stencil model's clusters need all of their workgroups resident at once, and eight processes'
    #  launches on ONE GPU would starve each other -- every process sizes its cluster grid for a share of the compute units)
    e = {"MUSE_BENCH_BACKEND": "gloo", "MUSE_BENCH_TRANSPORT": "shm", "MUSE_SHARED_GPU_RANKS": "16"}
    # (round 6: --nsims -- what this test checks is the eight-way deal, not the full job: eight processes time-slicing ONE GPU through
    #  1024 sims x N = 10^5 took ten minutes of the driver's GPU test step)
    d = run(["--gpus", "8", "--workload", "cfg4_fd_H", "--steps", "2", "--warmup", "1", "--nsims", "64"], e)
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and "8 ranks seen" in d["config"]["parallelism"]
    assert "513 MAP+score problems per step" in d["config"]["workload"] and "65 on this rank" in d["config"]["workload"]
    assert d["value"] > 0 and abs(d["value"] - 513 / (1e-3 * d["ms_per_step"])) < 1e-6 * d["value"]
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] <= 1
    d = run(["--gpus", "8", "--workload", "cfg5_smooth_1e5", "--steps", "2", "--warmup", "1", "--nsims", "32"], e)
    assert d["n_gpus"] == 8 and d["config"]["sims_per_step_total"] == 32 and "(4 on this rank)" in d["config"]["workload"]
    assert d["transports"]["shm"]["ranks_seen"] == 8
    assert d["value"] > 0 and abs(d["value"] - 32 / (1e-3 * d["ms_per_step"])) < 1e-6 * d["value"]


def test_bench_single_gpu_runs_of_the_8_gpu_workloads(gpu):
    d = run(["--workload", "cfg4_fd_H", "--steps", "8", "--warmup", "2"], {})
    assert d["n_gpus"] == 1 and "4097 on this rank" in d["config"]["workload"] and 0 < d["roofline"]["frac"] <= 1
    d = run(["--workload", "cfg5_smooth_1e5", "--steps", "3", "--warmup", "1"], {})
    assert d["n_gpus"] == 1 and d["config"]["sims_per_step_total"] == 1024 and d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] <= 1


def test_bench_default_line_carries_the_other_workloads_and_projections(gpu):
    """The full run (`python bench.py --full`: extras on; only the CPU baseline left out here): the other BASELINE
    workloads are timed inside it, the two 8-GPU workloads are projected, and the dependent path's 8-GPU share -- the sharded loop as
    ONE persistent launch through a one-rank communicator -- is in the line with both kinds of iteration told apart."""
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--min-seconds", "0", "--full",
                        "--no-cpu-baseline"],
                       env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    x = d["extra"]
    for w in ("funnel4_1e4", "noise_1e6", "smooth_1e5"):
        assert 0 < x["workloads"][w]["frac"] <= 1 and x["workloads"][w]["ms_per_step"] > 0, x["workloads"][w]
    assert x["workloads"]["noise_1e6"]["bound"] == "hbm" and x["workloads"]["funnel4_1e4"]["bound"] == "valu"
    sp = x["scale_projection"]
    assert sp["cfg5_smooth_1e5"]["projected_speedup_at_8_gpus"] > 4 and sp["cfg4_fd_H"]["projected_speedup_at_8_gpus"] > 2
    sh = x["muse_run_8gpu_share"]
    assert sh["elements_per_rank"] == 65 and sh["projected_speedup_at_8_gpus"] > 2
    # (a note, not an assertion -- the driver's box is shared: the persistent launch through the boards in device memory has been
    #  faster than through the host's board, and that faster than the host-driven loop, on every box so far)
    dev, hostboard, hostloop = (sh[k]["us_per_outer_iteration_steady"] for k in
                                ("sharded_loop_shm_1rank", "sharded_loop_host_board_shm_1rank", "sharded_host_loop_shm_1rank"))
    print(f"share iteration: device boards {dev:.1f} us, host board {hostboard:.1f} us, host-driven loop {hostloop:.1f} us")
    assert [sh[k]["loop_ran"] for k in ("sharded_loop_shm_1rank", "sharded_loop_host_board_shm_1rank", "sharded_host_loop_shm_1rank")] == ["device", "host", "none"]
    assert sh["board_handshake"]["device_handshake"] == 1 and sh["board_handshake"]["host_handshake"] == 1
    # round 6: the figures the driver's record keeps -- flat scalars of `config` and `roofline`
    c, r = d["config"], d["roofline"]
    for k in ("funnel4_ms", "funnel4_frac", "noise_1e6_ms", "noise_1e6_frac", "smooth_1e5_ms", "smooth_1e5_frac", "muse_iter_us", "muse_iter_steady_us",
              "share_iter_us", "proj_muse", "proj_cfg4", "proj_cfg5", "cfg4_whole_ms", "cfg4_share_ms", "handshake_device", "handshake_host"):
        assert isinstance(c[k], (int, float)) and c[k] > 0, (k, c.get(k))
    assert 0 < r["hbm_frac"] < 1 and 0 < r["frac_kernel_time"] <= 1 and r["frac_definition"].startswith("pipelined")
    assert set(sh["projected_by_regime"]) <= {"line_search", "converged_at_start"} and sh["projected_by_regime"]
    assert "line_search" in x["muse_run"]["by_regime"]


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(gpu, O, tmp_path):
    """`python bench.py --steps K --warmup W` without --full: EXACTLY K timed steps, the headline fields and nothing that takes a run
    of its own (no roofline leg, no extras, no CPU baseline); --dump-outputs writes the last timed step's scores and solver infos,
    which are the oracle's for the same 512 simulations (the same parity as tests/test_gpu_parity.py)."""
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["timed_rounds"] == 1 and d["unit"] == "sims/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["value"] - 512 / (1e-3 * d["ms_per_step"])) < 1e-6 * d["value"]
    assert abs(d["timed_seconds"] - 7e-3 * d["ms_per_step"]) < 1e-9
    assert not {"roofline", "extra", "cpu_baseline"} & set(d), sorted(d)
    g = np.load(out / "scores.npy")
    assert g.dtype == np.float64 and g.shape == (512, 1)
    go, _, io = O.map_and_score_batch("funnel", 10000, 0, 0, 512, [1.0], atol=1e-2, z0_mode=0, nthreads=8)
    for field in ("iterations", "f_calls", "status"):
        got = np.load(out / f"{field}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, io[field].astype(np.float64)), field
    np.testing.assert_allclose(g, go, rtol=1e-10)
