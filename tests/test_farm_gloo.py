"""world_size-2 gloo run of the N>1 path: sequence sharding, barrier-bracketed timing, MAX time / SUM work reduce.
The per-rank 'GPU work' is replaced by the CPU oracle on tiny frames (no GPU in this container)."""
import os
import sys

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__ as ge
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    orc = ge.load_oracle()
    W, H, nseq = 24, 16, 5
    mine = pkg.farm.shard(nseq, world, rank)
    engines = {s: orc.Oracle(pkg, W, H) for s in mine}
    frames = {s: pkg.synth.render_frame(W, H, 0, seed=100 + s) for s in mine}
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=2)
    checks = {}

    def step(i):
        px = 0
        for s in mine:
            out = engines[s].denoise(*frames[s], p)
            checks[s] = float(out.sum())
            px += W * H
        return px

    calls = [0]

    def counted(i):
        calls[0] += 1
        return step(i)

    busy = dist.new_group(backend="gloo")      # (a collective itself: both ranks are here)
    if rank == 1:
        import time
        time.sleep(0.3)           # rank 0 arrives first and must keep stepping (untimed) until rank 1 is there
    dt, units = pkg.farm.timed_region(counted, steps=3, warmup=1, sync_fn=lambda: None, dist=dist, busy_group=busy)
    q.put((rank, mine, dt, units, checks, calls[0]))
    dist.destroy_process_group()


def test_two_rank_farm():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort()
    assert sorted(res[0][1] + res[1][1]) == [0, 1, 2, 3, 4]          # every sequence owned once
    assert res[0][2] == res[1][2] > 0                                 # both ranks report the MAX time
    assert res[0][3] == res[1][3] == 3 * 5 * 24 * 16                  # SUM of work over ranks = all sequences x steps
    # a sequence gives the same result whichever rank runs it
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package(); orc = ge.load_oracle()
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=2)
    # the rank that arrived early kept its engine busy with untimed steps while it waited (busy_group); only 3 steps were timed on both
    assert res[0][5] > res[1][5] >= 4 and res[0][3] == 3 * 5 * 24 * 16
    for (_, mine, _, _, checks, ncalls) in res:
        for s in mine:
            o = orc.Oracle(pkg, 24, 16)
            fr = pkg.synth.render_frame(24, 16, 0, seed=100 + s)
            for _ in range(ncalls):          # warm-up + the untimed steps of the rendezvous + the 3 timed ones
                out = o.denoise(*fr, p)
            o.free()
            assert np.isclose(float(out.sum()), checks[s], rtol=0, atol=0)


def test_bench_refuses_to_run_without_a_gpu():
    """bench.py measures the HIP path only: on a host without a GPU it must stop with a clear message, not fall back."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU present")
    from conftest import ROOT
    import os
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0
    assert "needs a GPU" in (r.stderr + r.stdout)


import pytest  # noqa: E402


@pytest.mark.gpu
def test_bench_distributed_branch_runs_with_one_rank_on_rccl():
    """The multi-GPU branch of bench.py (RCCL process group on `nccl`, barrier + MAX / SUM all-reduces around the timed region)
    as far as a one-GPU box can exercise it: SVGF_BENCH_FORCE_DIST=1 takes that branch with world size 1.  The JSON line must
    carry BASELINE's metric and the same fields as the plain run."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, SVGF_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1")
    env.pop("MASTER_PORT", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline",
                        "--min-warmup-seconds", "0.1", "--cadence-frames", "16"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"].startswith("SVGF Mpixels/s (full pipeline) at 1080p") and line["unit"] == "Mpixels/s"
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["scaling"] == "weak" and line["value"] > 100
    assert 0 < line["roofline"]["frac"] < 1 and line["config"]["parallelism"] == "replicas1"
    # the line says which state of the GPU was timed and what it rests on
    assert line["state"] == "sustained" and line["cold_ms_per_step"] > line["ms_per_step"] > 0
    assert len(line["per_rank"]) == 1 and line["per_rank"][0]["rank"] == 0 and line["per_rank"][0]["device"] == 0
    vv = line["roofline"]["valu_view"]
    assert vv["simd_instruction_active_pmc"] is None or 0.5 < vv["simd_instruction_active_pmc"] <= 1.01      # a PMC record or nothing: never a literal
    assert "formula" in vv["fp32_tflops_isolated_is"] and "formula" in line["roofline"]["transcendental_gops_isolated_is"]
    # the benchmark creates its context pipelined and decides by a trial (regions of --steps frames, medians, >= 3 %) which way the timed
    # steps run; the line carries the trial, the other leg from an identical region, and what the library's queue probe said
    tr = line["frame_pipeline_trial"]
    assert line["frame_pipeline_status"] == 1 and tr and len(tr["pipelined_ms"]) == len(tr["ordered_ms"]) >= 3
    assert line["frame_pipeline"] == (tr["pipelined_median_ms"] <= 0.97 * tr["ordered_median_ms"])
    other = line["ordered"] if line["frame_pipeline"] else line["pipelined"]
    assert other["ms_per_step"] > 0 and line["first_frame_ms"] < 50
    # roofline = the dominant kernel's OWN figure (ordered frames, one kernel at a time): frac x peak x duration = the algorithmic bytes
    rf = line["roofline"]
    assert abs(rf["frac"] * rf["peak"] * 1e9 * rf["mean_launch_us"] * 1e-6 - 56.0 * 1920 * 1080) <= 0.01 * 56.0 * 1920 * 1080
    assert rf["timed_region"]["mean_launch_us"] >= 0.9 * rf["mean_launch_us"] and rf["timed_region"]["launches_timed"] >= 5
    # (5 timed steps: the one profiled frame is the first behind a synchronisation and may run alone for a while; the steady-state
    # figure, ~1.7 kernels in flight, is bench.py's default run — here only the field's presence and sanity are checked)
    assert rf["timed_region"]["kernels_in_flight_mean"] > 0.5 and 0 < rf["timed_region"]["frac"] < 1
    # the state a renderer lives in: one frame per 1/60 s, GPU idle in between
    cd = line["cadence"]
    assert cd["hz"] == 60.0 and cd["ms_per_step"] > 0.9 * line["ms_per_step"] and cd["frames"] >= 8


@pytest.mark.gpu
def test_bench_launcher_two_ranks_sharing_one_gpu():
    """`python bench.py --gpus 2` as far as a one-GPU box can take it (SVGF_BENCH_SHARE_DEVICE=1): the launcher spawns two ranks,
    each creates its own context (both on device 0), the ranks rendezvous over gloo, the timed region is bracketed by the barrier
    and reduced with MAX (time) / SUM (pixels), and exactly ONE JSON line comes out, from rank 0, with n_gpus = 2 and both
    ranks' pixels in `value`.  (Real multi-GPU runs use one GPU per rank over RCCL: the branch the one-rank test above takes.)"""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, SVGF_BENCH_SHARE_DEVICE="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline",
                        "--min-warmup-seconds", "0.1", "--latency-calls", "50"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"{len(lines)} JSON lines from a 2-rank run"
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 6 and line["scaling"] == "weak"
    assert line["config"]["parallelism"].startswith("replicas2")
    # both ranks' pixels over the slower rank's time: two contexts time-slicing one GPU land near (not above ~1.2x) one context's rate
    px_per_step = 1920 * 1080
    assert abs(line["value"] * 1e6 * line["ms_per_step"] * 1e-3 - 2 * px_per_step) <= 0.01 * 2 * px_per_step
    assert "cpu_baseline" not in line and line["latency_ms_sync"] > 0
    # one entry per rank: its own clock around its own steps, its device, a CPU slice disjoint from the other rank's
    pr = line["per_rank"]
    assert [r_["rank"] for r_ in pr] == [0, 1] and all(r_["device"] == 0 for r_ in pr)
    assert all(0 < r_["ms_per_step"] <= line["ms_per_step"] * 1.001 for r_ in pr)
    assert pr[0]["cpus"] and pr[1]["cpus"] and not (set(pr[0]["cpus"]) & set(pr[1]["cpus"])) or len(os.sched_getaffinity(0)) < 2


@pytest.mark.gpu
def test_bench_launcher_eight_ranks_sharing_one_gpu_on_configs4():
    """BASELINE configs[4]'s command, `python bench.py --gpus 8 --config 4k-room`, as far as ONE GPU can take it (SVGF_BENCH_SHARE_DEVICE=1):
    the launcher spawns eight ranks, they rendezvous (gloo here; RCCL with a GPU each), every rank pins itself to its own slice of the
    CPUs the container may use, ray-casts room.txt at 3840x2160 with the device producer, creates its own 4K context (eight of them fit
    one device with room to spare: 8 x ~4 GB of 288), and ONE JSON line with eight per_rank entries comes out.  No 1 -> 8 scaling
    number is claimed anywhere: no run of this repository has had two GPUs."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, SVGF_BENCH_SHARE_DEVICE="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--config", "4k-room", "--steps", "3", "--warmup", "1", "--full",
                        "--min-warmup-seconds", "0.05", "--latency-calls", "50", "--trial-reps", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"{len(lines)} JSON lines from an 8-rank run"
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["steps"] == 3 and line["scaling"] == "weak" and line["config"]["name"] == "4k-room"
    assert line["config"]["width"] == 3840 and line["config"]["parallelism"].startswith("replicas8")
    px = 3840 * 2160
    assert abs(line["value"] * 1e6 * line["ms_per_step"] * 1e-3 - 8 * px) <= 0.01 * 8 * px      # all ranks' pixels over the slowest rank's time
    pr = line["per_rank"]
    assert [e["rank"] for e in pr] == list(range(8)) and all(e["device"] == 0 for e in pr)
    assert all(0 < e["ms_per_step"] <= line["ms_per_step"] * 1.001 for e in pr)
    ncpu = len(os.sched_getaffinity(0))
    if ncpu >= 8:
        sets = [set(e["cpus"]) for e in pr]
        assert all(sets) and all(not (sets[i] & sets[j]) for i in range(8) for j in range(i)), sets
    assert "cpu_baseline" not in line and line["cadence"] is None
