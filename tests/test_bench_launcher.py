"""bench.py as the driver runs it: `python bench.py --gpus N` must start N ranks itself, and under
`python -m torch.distributed.run` it must be one of the existing ranks.  No GPU here, so the ranks run `--dry-run`:
the launcher, the rendezvous on 127.0.0.1, the loss gather in pose order and the max-over-ranks timing are the real
code; only the kernels are skipped."""
import json
import os
import socket
import subprocess
import sys
import time
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "4", "--poses", "3"], env=_env(),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2 and out["dry_run"] is True
    assert len(out["per_rank_ms_per_step"]) == 2
    assert out["ms_per_step"] == pytest.approx(max(out["per_rank_ms_per_step"]))      # MAX over ranks


@pytest.mark.parametrize("steps,every", [(11, 4), (8, 8), (3, 8), (5, 1)])
def test_bucketed_loss_gather_delivers_every_steps_losses_in_pose_order(steps, every):
    """N > 1: the losses of `every` consecutive steps leave in one all_gather; a part-filled ring goes out at the end.
    The dry run asserts that the last step's losses of every rank come back in pose order (rank-major)."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", str(steps), "--poses", "3",
                        "--gather-every", str(every)], env=_env(), capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert _json_line(r.stdout)["n_gpus"] == 2


def test_default_scaling_is_strong_config_4_over_the_ranks():
    """P = 256 fixed, P / k poses per GPU.  `--gpus 2` must shard 128 poses per rank, in pose order
    (the dry run asserts that the gathered stand-in losses come back as pose 0..255), and say "strong"."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "3"], env=_env(),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert out["scaling"] == "strong" and out["poses_total"] == 256 and out["poses_per_rank"] == [128, 128]
    assert out["config"]["workload"] == "BASELINE config 4 at 2 of 8 GPUs"
    # weak on request: --poses per GPU whatever N
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "3", "--scaling", "weak", "--poses", "5"],
                       env=_env(), capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert out["scaling"] == "weak" and out["poses_total"] == 10 and out["poses_per_rank"] == [5, 5]


def test_plan_poses_and_one_gpu_default():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args([])
    assert bench.plan_poses(a, 1) == ("weak", 32, 32)                 # N = 1: BASELINE config 3
    assert [bench.plan_poses(a, k)[1:] for k in (2, 4, 8)] == [(256, 128), (256, 64), (256, 32)]
    assert bench.plan_poses(bench.parse_args(["--scaling", "strong"]), 1) == ("strong", 256, 256)
    with pytest.raises(SystemExit):
        bench.plan_poses(bench.parse_args(["--poses-total", "250"]), 4)
    assert a.gather_every == 1 and a.steps >= 200                     # ADVICE r2 / VERDICT r2 item 9


def test_launcher_counts_gpus_without_touching_hip(tmp_path):
    """the launcher must not call torch.cuda.  The count comes from the visibility variables / KFD sysfs."""
    sys.path.insert(0, ROOT)
    import bench
    nodes = tmp_path / "nodes"
    for i, simd in enumerate((0, 0, 1024, 1024, 1024)):                # two CPU nodes, three GPUs
        (nodes / str(i)).mkdir(parents=True)
        (nodes / str(i) / "properties").write_text(f"cpu_cores_count 0\nsimd_count {simd}\n")
    assert bench.visible_gpus({}, str(nodes)) == 3
    assert bench.visible_gpus({"HIP_VISIBLE_DEVICES": "0,1"}, str(nodes)) == 2
    assert bench.visible_gpus({"ROCR_VISIBLE_DEVICES": "0,1,2,3,4,5"}, str(nodes)) == 3
    assert bench.visible_gpus({}, str(tmp_path / "missing")) is None
    assert bench.visible_gpus({"HIP_VISIBLE_DEVICES": "3"}, str(tmp_path / "missing")) == 1
    import inspect
    assert "torch" not in inspect.getsource(bench.launch_ranks)


def test_sigterm_to_the_launcher_takes_the_ranks_down():
    """a SIGTERM (or Ctrl-C) to the launcher must not orphan the ranks."""
    import signal
    p = subprocess.Popen([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "2000000", "--poses-total", "2"], env=_env(),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    time.sleep(6)
    kids = subprocess.run(["pgrep", "-P", str(p.pid)], capture_output=True, text=True).stdout.split()
    assert len(kids) == 2, kids
    p.send_signal(signal.SIGTERM)
    p.wait(timeout=60)
    assert p.returncode != 0
    time.sleep(0.5)
    for k in kids:
        assert not os.path.exists(f"/proc/{k}") or open(f"/proc/{k}/stat").read().split()[2] == "Z", k


def test_ring_helpers():
    sys.path.insert(0, ROOT)
    import torch

    import bench
    assert [bench.ring_slot(k, 4) for k in (0, 3, 4, 7, 8)] == [(0, 0), (3, 0), (0, 1), (3, 1), (0, 0)]
    world, K, P = 3, 4, 2
    g = torch.arange(world * K * P, dtype=torch.float32)     # rank-major, then slot, then pose
    assert bench.losses_of_step(g, world, K, P, 6).tolist() == [4.0, 5.0, 12.0, 13.0, 20.0, 21.0]   # slot 6 % 4 = 2


def test_under_torchrun_it_is_a_rank_not_a_launcher():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--dry-run",
                        "--steps", "2"], env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2


def test_a_failing_rank_fails_the_launcher_and_stops_the_others():
    t0 = time.time()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--fail-rank", "1"], env=_env(),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode != 0
    assert "rank 1 exited with 3" in r.stderr
    assert time.time() - t0 < 120            # rank 0 was stopped, not left waiting in the rendezvous


def test_single_gpu_default_does_not_spawn():
    r = subprocess.run([sys.executable, BENCH, "--dry-run", "--steps", "2"], env=_env(), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert _json_line(r.stdout)["n_gpus"] == 1


def test_labels_and_pmc_lookup_follow_the_workload(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args([])
    assert bench.config_label(a, 1) == "BASELINE config 3"
    assert bench.config_label(a, 8) == "BASELINE config 4"
    assert bench.config_label(a, 2) == "BASELINE config 4 at 2 of 8 GPUs"
    # 256 poses on ONE GPU is the k = 1 leg of config 4's scaling curve, not a "custom workload" 
    assert bench.config_label(bench.parse_args(["--scaling", "strong"]), 1) == "BASELINE config 4 at 1 of 8 GPUs"
    assert bench.config_label(bench.parse_args(["--poses", "256"]), 1) == "BASELINE config 4 at 1 of 8 GPUs"
    assert "weak" in bench.config_label(bench.parse_args(["--scaling", "weak"]), 4)
    a5 = bench.parse_args(["--n", "512", "--rays", "512", "--samples", "1024", "--poses", "8"])
    assert "config 5" in bench.config_label(a5, 1) and "config 3" not in bench.config_label(a5, 1)
    odd = bench.parse_args(["--n", "512"])
    assert "custom" in bench.config_label(odd, 1)            # a 512^3 run is never labelled config 3
    # the PMC summary speaks for a run only when volume, poses, rays, samples, start, sampler and layout all match
    prof = tmp_path / "profiles"
    prof.mkdir()
    key = bench.workload_key(a)
    (prof / "r02_pmc_c3.json").write_text(json.dumps({"workload": key, "kernels": {"k": {"hbm_bytes_per_launch": 7}}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.find_pmc_summary(key)[1]["kernels"]["k"]["hbm_bytes_per_launch"] == 7
    assert bench.find_pmc_summary(bench.workload_key(a5)) is None
    assert bench.find_pmc_summary(dict(key, n=512)) is None


@pytest.mark.gpu
def test_two_ranks_on_the_gpu_box_strong_scaling_line():
    """The N > 1 worker end to end on real kernels: `bench.py --gpus 2 --dist-backend gloo` (both ranks on cuda:0, the
    collectives through gloo -- RCCL refuses two ranks on one device) shards config 4's 256 poses 128 / 128, gathers the
    losses in pose order, verifies frames and gathered losses against the oracle and reports the strong / weak legs."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dist-backend", "gloo", "--steps", "5", "--warmup", "2",
                        "--no-cpu-baseline"], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2 and out["scaling"] == "strong"
    assert out["config"]["poses_total"] == 256 and out["config"]["poses_per_gpu"] == 128
    assert out["config"]["workload"].startswith("BASELINE config 4 at 2 of 8 GPUs")
    v = out["verified"]
    assert v["ok"] and 255 in [x["pose"] for x in v["losses"]]          # the LAST rank's last pose came back in place
    assert out["strong"]["one_gpu"]["poses_total"] == 256 and out["strong"]["speedup_vs_one_gpu"] > 0
    assert out["weak"]["poses_per_gpu"] == 32 and out["value"] > 0
    assert out["roofline"]["kernel"] in ("render_bwd_kernel", "scatter_patch_kernel") and out["roofline"]["algorithmic"]["GBs"] > 0


def test_gpu_numa_cpus_from_sysfs(tmp_path):
    """bench.gpu_numa_cpus: rank -> KFD GPU node -> render minor -> PCI device's NUMA node -> its CPU list, all from (a fake)
    sysfs; None whenever the chain breaks or the devices are re-ordered by a *_VISIBLE_DEVICES variable."""
    import bench
    nodes, drm, numa = tmp_path / "nodes", tmp_path / "drm", tmp_path / "numa"
    for i, (simd, minor) in enumerate([(0, -1), (0, -1), (256, 128), (256, 129), (256, 130)]):
        (nodes / str(i)).mkdir(parents=True)
        (nodes / str(i) / "properties").write_text(f"cpu_cores_count {0 if simd else 64}\nsimd_count {simd}\ndrm_render_minor {minor}\n")
    for minor, node in ((128, 0), (129, 1), (130, -1)):
        (drm / f"renderD{minor}" / "device").mkdir(parents=True)
        (drm / f"renderD{minor}" / "device" / "numa_node").write_text(f"{node}\n")
    for k, cl in ((0, "0-3,16-19"), (1, "4-7,20")):
        (numa / f"node{k}").mkdir(parents=True)
        (numa / f"node{k}" / "cpulist").write_text(cl + "\n")
    kw = dict(kfd_nodes=str(nodes), drm=str(drm), numa=str(numa))
    assert bench.gpu_numa_cpus(0, {}, **kw) == {0, 1, 2, 3, 16, 17, 18, 19}
    assert bench.gpu_numa_cpus(1, {}, **kw) == {4, 5, 6, 7, 20}
    assert bench.gpu_numa_cpus(2, {}, **kw) is None                     # numa_node -1
    assert bench.gpu_numa_cpus(3, {}, **kw) is None                     # no such GPU
    assert bench.gpu_numa_cpus(0, {"HIP_VISIBLE_DEVICES": "1,0"}, **kw) is None
    assert bench.gpu_numa_cpus(0, {}, kfd_nodes=str(tmp_path / "missing"), drm=str(drm), numa=str(numa)) is None


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(tmp_path):
    """bench.dump_outputs: every array as <name>.npy within the byte budget; the small ones whole, the one that does not fit
    as its values at a fixed set of increasing flat indices, the same set on every call."""
    import numpy as np
    import torch
    import bench
    arrays = {"loss": torch.arange(4, dtype=torch.float32), "grad": torch.arange(60, dtype=torch.float64).reshape(3, 20),
              "big": torch.arange(2000, dtype=torch.float32).reshape(20, 100)}
    budget = 128 * 3 + 4 * 4 + 8 * 60 + 4 * 500
    info = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "grad.npy", "loss.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    for name in ("loss", "grad"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert info[name]["sampled"] is None and a.dtype == arrays[name].numpy().dtype
        np.testing.assert_array_equal(a, arrays[name].numpy())
    big = np.load(tmp_path / "a" / "big.npy")
    assert info["big"] == {"shape": [20, 100], "dtype": "float32", "sampled": 500} and big.shape == (500,)
    assert np.all(np.diff(big) > 0) and big[0] >= 0 and big[-1] < 2000        # values = their flat indices here
    np.testing.assert_array_equal(big, np.load(tmp_path / "b" / "big.npy"))


def test_steps_below_one_are_refused():
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


@pytest.mark.gpu
def test_dump_outputs_are_what_the_last_timed_step_computed(tmp_path):
    """`bench.py --dump-outputs DIR` on a small workload: the frame, the per-pose losses (= sum of the frame's squares) and
    the three gradients of the timed step, whole, and a result line that says K steps were timed."""
    import numpy as np
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "2", "--prewarm-ms", "0",
                        "--n", "64", "--poses", "2", "--rays", "16", "--samples", "64", "--no-cpu-baseline", "--no-callers",
                        "--no-scaling-legs", "--dump-outputs", str(out_dir)], env=_env(), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json_line(r.stdout)
    assert out["steps"] == 7 and out["ms_per_step"] > 0 and out["verified"]["ok"]
    shapes = {"frame": [2, 16, 64], "loss": [2], "grad_sources": [2, 3], "grad_directions": [2, 16, 3],
              "grad_volume": [64, 64, 64]}
    assert {k: v["shape"] for k, v in out["dumped_outputs"]["arrays"].items()} == shapes
    got = {k: np.load(out_dir / f"{k}.npy") for k in shapes}
    for k, shape in shapes.items():
        assert list(got[k].shape) == shape and got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
    want = (got["frame"].astype(np.float64) ** 2).sum(axis=(1, 2))
    np.testing.assert_allclose(got["loss"], want, rtol=1e-4)
    assert np.abs(got["grad_volume"]).max() > 0 and np.abs(got["grad_sources"]).max() > 0
