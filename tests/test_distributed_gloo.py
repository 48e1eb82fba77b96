"""gloo tests of the N>1 path.  CPU (logic only): the renderer is injected -- here the CPU oracle --, and the sparse
gradient collective runs over many steps against a numpy restatement of the hand-back (oracle/handback.py); on GPUs the
same code runs with backend 'nccl' = RCCL.  GPU: two ranks of the real kernels against float64 autograd."""
import os
import socket
import sys
import time
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT_TIMEOUT = timedelta(seconds=60)      # a rank that waits longer for its peers fails instead of hanging the suite


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, P, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=INIT_TIMEOUT)
    from diffus_amd.distributed import render_sharded, shard_bounds
    from diffus_amd.phantom import phantom, pose_ring
    from oracle import autograd_ref as ar

    n, R, S, alpha = 32, 6, 40, 1e-3
    vol = torch.from_numpy(phantom(n)).double().requires_grad_(True)
    src, dirs = pose_ring(n, P, R)
    src_t = torch.from_numpy(src).double().requires_grad_(True)
    dirs_t = torch.from_numpy(dirs).double()

    def render_fn(v, s, d):
        return torch.stack([ar.render(v, s[p], d[p], S, alpha, 0, "trilinear") for p in range(s.shape[0])]) \
            if s.shape[0] else torch.zeros((0, R, S), dtype=torch.float64)

    frames, losses, losses_all = render_sharded(render_fn, vol, src_t, dirs_t, lambda f: (f ** 2).sum((1, 2)))
    if losses.numel():
        losses.sum().backward()
    gvol = vol.grad if vol.grad is not None else torch.zeros_like(vol)
    from diffus_amd.distributed import allreduce_volume_grad
    allreduce_volume_grad(gvol)
    lo, hi = shard_bounds(P, rank, world)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), losses_all=losses_all.numpy(), gvol=gvol.detach().numpy(),
             gsrc=(src_t.grad.numpy() if src_t.grad is not None else np.zeros((P, 3))), lo=lo, hi=hi)
    dist.barrier()
    dist.destroy_process_group()


def _single(P):
    sys.path.insert(0, ROOT)
    from diffus_amd.phantom import phantom, pose_ring
    from oracle import autograd_ref as ar
    n, R, S, alpha = 32, 6, 40, 1e-3
    vol = torch.from_numpy(phantom(n)).double().requires_grad_(True)
    src, dirs = pose_ring(n, P, R)
    s = torch.from_numpy(src).double().requires_grad_(True)
    d = torch.from_numpy(dirs).double()
    losses = torch.stack([(ar.render(vol, s[p], d[p], S, alpha, 0, "trilinear") ** 2).sum() for p in range(P)])
    losses.sum().backward()
    return losses.detach().numpy(), vol.grad.numpy(), s.grad.numpy()


def _run(P, tmp_path, world=2):
    port = _free_port()
    mp.spawn(_worker, args=(world, port, P, str(tmp_path)), nprocs=world, join=True)
    ref_l, ref_gv, ref_gs = _single(P)
    outs = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]
    for o in outs:
        np.testing.assert_allclose(o["losses_all"], ref_l, rtol=1e-12)       # every rank sees all P losses, in order
        np.testing.assert_allclose(o["gvol"], ref_gv, rtol=1e-9, atol=1e-18)  # all-reduced shared-volume gradient
    gs = np.zeros_like(ref_gs)
    for o in outs:                                                             # pose gradients stay on the owning rank
        lo, hi = int(o["lo"]), int(o["hi"])
        gs[lo:hi] = o["gsrc"][lo:hi]
        mask = np.ones(P, bool); mask[lo:hi] = False
        assert np.all(o["gsrc"][mask] == 0)
    np.testing.assert_allclose(gs, ref_gs, rtol=1e-9)


def test_two_ranks_even_split(tmp_path):
    _run(4, tmp_path)


def test_two_ranks_ragged_split(tmp_path):
    _run(3, tmp_path)


@pytest.mark.parametrize("P,world", [(5, 3), (8, 4), (3, 4)])
def test_more_ranks_than_two(tmp_path, P, world):
    """Worlds 3 and 4, ragged and even; (3, 4): a rank with an empty shard still joins both collectives."""
    _run(P, tmp_path, world)


def _sparse_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=INIT_TIMEOUT)
    from diffus_amd.distributed import allreduce_box, allreduce_touched, allreduce_volume_grad
    g = torch.Generator().manual_seed(100 + rank)
    # (a) one slice of a canonical gradient
    shape = (12, 10, 8)
    gv = torch.randn(shape, generator=g)
    dense = gv.clone()
    box = ((0, 12), (0, 10), (3, 4))
    moved_box = allreduce_box(gv, box)
    allreduce_volume_grad(dense)
    # (b) the bricked scratch + touched flags of a scatter: each rank touches its own random third of 60 bricks
    nb = 60
    touched = (torch.rand(nb, generator=g) < 0.33).to(torch.int32)
    touched[7] = 2 if rank == 0 else 0                          # a flag 2 ("stale", left by a PERSISTENT flush) is not live scratch
    touched[11] = 2 if rank == 0 else 1                         # stale on one rank, live on the other: live on both afterwards
    bricks = torch.randn(nb, 32, generator=g) * (touched == 1).unsqueeze(1)
    want = bricks.clone()
    allreduce_volume_grad(want)
    t_before = touched.clone()
    moved_t = allreduce_touched(bricks.view(-1), touched)
    np.savez(os.path.join(out_dir, f"s{rank}.npz"), gv=gv.numpy(), dense=dense.numpy(), own=torch.randn(shape, generator=torch.Generator().manual_seed(100 + rank)).numpy(),
             bricks=bricks.numpy(), want=want.numpy(), touched=touched.numpy(), t_before=t_before.numpy(), moved_box=moved_box, moved_t=moved_t)
    dist.barrier()
    dist.destroy_process_group()


def test_sparse_allreduce_of_a_shared_volume_gradient_live_union(tmp_path):
    """allreduce_box / allreduce_touched against the dense all_reduce of the whole tensor (world 2, gloo): same sums where a
    step can have written, nothing else touched, a fraction of the bytes (SURVEY §8e "Collective"; the reference's training
    loop learns one slice: `[DEMO] Train MRI to Impedance MLP - GPU` cell 16).  allreduce_touched moves the LIVE union
    (flag 1): a stale flag (2) on one rank only is not moved and stays as it was; stale on one rank and live on the other
    becomes live on both."""
    world, port = 2, _free_port()
    mp.spawn(_sparse_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    outs = [np.load(os.path.join(tmp_path, f"s{r}.npz")) for r in range(world)]
    union = (outs[0]["t_before"] == 1) | (outs[1]["t_before"] == 1)                         # the LIVE union (flag 1)
    assert not union[7] and union[11]
    for r, o in enumerate(outs):
        np.testing.assert_allclose(o["gv"][:, :, 3], o["dense"][:, :, 3], rtol=1e-6)        # the slice: summed over the ranks
        rest = np.ones(o["gv"].shape, bool); rest[:, :, 3] = False
        assert np.array_equal(o["gv"][rest], o["own"][rest])                                 # everything else: this rank's own values
        assert int(o["moved_box"]) == 12 * 10 * 4
        np.testing.assert_allclose(o["bricks"], o["want"], rtol=1e-6, atol=1e-7)             # bricked scratch: the dense sum
        assert np.array_equal(o["touched"] == 1, union)                                     # every rank flushes the live union
        assert np.all(o["touched"][(o["t_before"] != 1) & union] == 1)                     # 0 and 2 alike become live
        assert np.array_equal(o["touched"][~union], o["t_before"][~union])                  # stale flags stay per rank
        assert np.all(o["bricks"][~union] == 0)                                              # nothing written outside it
        assert int(o["moved_t"]) == 60 + int(union.sum()) * 32 * 4 < 60 * 32 * 4
    # brick 7 (stale on rank 0 only) is not moved: rank 0 keeps its 2 (its flush clears the brick in `out`), rank 1 its 0
    assert int(outs[0]["touched"][7]) == 2 and int(outs[1]["touched"][7]) == 0
    assert int(outs[0]["touched"][11]) == 1 and int(outs[1]["touched"][11]) == 1


# -- allreduce_touched over many steps, with the hand-back restated in numpy (oracle/handback.py) -------------------------
MULTISTEP_SHAPES = [(9, 10, 7), (12, 8, 6), (5, 3, 1)]
MULTISTEP_STEPS = 10
# brick 0 walks through every transition whatever the seed: live on every rank, then on rank 0 alone (stale on the others),
# on none (stale everywhere), on the last rank alone, ...
_BRICK0 = ("all", "first", "none", "last", "none", "all", "first", "none")


def _touches(world, shape, mode, step, rank):
    """(bricks this rank's scatter touches at `step`, the values it adds into them): seeded, the same in every process."""
    from oracle import handback as hb
    nb = hb.brick_count(shape)
    rng = np.random.default_rng([world, *shape, mode, step, rank])
    pick = rng.random(nb) < (0.15, 0.5, 0.3, 0.05)[step % 4]
    which = _BRICK0[step % len(_BRICK0)]
    pick[0] = which == "all" or (which == "first" and rank == 0) or (which == "last" and rank == world - 1)
    vals = rng.standard_normal((nb, 32)).astype(np.float32)          # the 32 slots, those outside the volume included
    return pick, vals


def _multistep_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=INIT_TIMEOUT)
    from diffus_amd.distributed import allreduce_touched
    from oracle import handback as hb
    for shape in MULTISTEP_SHAPES:
        for mode in (hb.PERSISTENT, hb.STORE):
            nb = hb.brick_count(shape)
            scratch = np.zeros(nb * 32, np.float32)
            touched = np.zeros(nb, np.int32)
            out = np.zeros(shape, np.float32)
            rec = {k: [] for k in ("pre", "flags", "scratch", "out", "moved")}
            for step in range(MULTISTEP_STEPS):
                pick, vals = _touches(world, shape, mode, step, rank)
                scratch.reshape(nb, 32)[pick] += vals[pick]                 # the scatter: adds, and sets flag 1
                touched[pick] = 1
                rec["pre"].append(touched.copy())
                if mode == hb.STORE:
                    out[...] = 0.0                                          # CapturedStep.zero_grad before a STORE hand-back
                rec["moved"].append(allreduce_touched(torch.from_numpy(scratch), torch.from_numpy(touched)))
                hb.flush(scratch, touched, out, mode)
                rec["flags"].append(touched.copy())
                rec["scratch"].append(scratch.copy())
                rec["out"].append(out.copy())
            np.savez(os.path.join(out_dir, f"m{rank}_{'x'.join(map(str, shape))}_{mode}.npz"),
                     **{k: np.stack(v) for k, v in rec.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def multistep_runs(tmp_path_factory):
    """world -> the directory its ranks wrote their per-step records to; each world is spawned once for every case."""
    runs = {}

    def get(world):
        if world not in runs:
            d = tmp_path_factory.mktemp(f"multistep{world}")
            mp.spawn(_multistep_worker, args=(world, _free_port(), str(d)), nprocs=world, join=True)
            runs[world] = d
        return runs[world]
    return get


@pytest.mark.parametrize("shape", MULTISTEP_SHAPES)
@pytest.mark.parametrize("mode", ["persistent", "store"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_allreduce_touched_over_steps(multistep_runs, world, mode, shape):
    """Every step, every rank touches its own random bricks, calls allreduce_touched, then flushes (the numpy model of
    diffus_gradbuf_flush).  After every step: `out` is the dense sum of that step's contributions of all ranks and the same
    bits on every rank, the scratch is all-zero, the flags are 2 x (live union) (PERSISTENT) or 0 (STORE), and the
    collective moved the flags plus the live union's bricks.  The schedule is checked to contain every flag transition:
    (a) stale on one rank and live on another, (b) stale on every rank, (c) live on several ranks, (d) live on one."""
    from oracle import handback as hb
    code = {"persistent": hb.PERSISTENT, "store": hb.STORE}[mode]
    d = multistep_runs(world)
    recs = [np.load(os.path.join(d, f"m{r}_{'x'.join(map(str, shape))}_{code}.npz")) for r in range(world)]
    nb = hb.brick_count(shape)
    seen = dict(a=0, b=0, c=0, d=0)
    problems = []
    for step in range(MULTISTEP_STEPS):
        contrib = np.zeros((nb, 32))
        for r in range(world):
            pick, vals = _touches(world, shape, code, step, r)
            contrib[pick] += vals[pick]
        want = hb.unbrick(contrib, shape)
        pre = np.stack([rc["pre"][step] for rc in recs])
        live_n, stale_n = (pre == 1).sum(0), (pre == 2).sum(0)
        union = live_n > 0
        seen["a"] += int(((stale_n > 0) & (live_n > 0)).sum())
        seen["b"] += int((stale_n == world).sum())
        seen["c"] += int((live_n >= 2).sum())
        seen["d"] += int((live_n == 1).sum())
        for r, rc in enumerate(recs):
            out = rc["out"][step]
            tag = f"step {step} rank {r}"
            if world == 2:
                ok = np.array_equal(out, want.astype(np.float32))            # a + b: one rounding, exact
            else:
                ok = np.allclose(out, want, rtol=1e-6, atol=1e-6 * float(np.abs(want).max()))
            if not ok:
                bad = int((out != want.astype(np.float32)).sum())
                problems.append(f"{tag}: lost contribution: `out` differs from the sum over the ranks at {bad} voxels")
            if np.any(rc["scratch"][step] != 0):
                problems.append(f"{tag}: dirty scratch: {int((rc['scratch'][step] != 0).sum())} non-zero floats after the flush")
            flags = rc["flags"][step]
            wf = 2 * union.astype(np.int32) if code == hb.PERSISTENT else np.zeros(nb, np.int32)
            if not np.array_equal(flags, wf):
                problems.append(f"{tag}: flags {np.unique(flags).tolist()} are not {'2 x live union' if code == hb.PERSISTENT else '0'}"
                                f" at {int((flags != wf).sum())} bricks")
            if not np.array_equal(out.view(np.uint32), recs[0]["out"][step].view(np.uint32)):
                problems.append(f"{tag}: `out` differs from rank 0's")
            if int(rc["moved"][step]) != nb + 128 * int(union.sum()):
                problems.append(f"{tag}: moved {int(rc['moved'][step])} bytes, the live union needs {nb + 128 * int(union.sum())}")
    assert not problems, "\n".join(problems[:12] + ([f"... {len(problems) - 12} more"] if len(problems) > 12 else []))
    if code == hb.PERSISTENT:
        assert seen["a"] > 0 and seen["b"] > 0, seen
    else:
        assert seen["a"] == 0 and seen["b"] == 0, seen                       # a STORE hand-back leaves no stale flag
    assert seen["c"] > 0 and seen["d"] > 0, seen


# -- two ranks of the real kernels (GPU) ------------------------------------------------------------------------------------
# Both ranks on device 0, backend gloo on HIP tensors (what the sparse collective does is backend-independent; one device
# suffices).  Each rank's fans move every step, so that bricks one rank's fans left stale are reached by the other
# rank's fans at the next step.
GPU_BACKEND = "gloo"
GPU_SCHEDULE = ([[0, 1], [5], [5], [2, 9], [3], [0, 1]],
                [[5, 6], [0, 1], [7], [5], [3, 4], [8]])
GPU_CASES = [(sampler, layout, persistent) for sampler in ("trilinear", "nearest") for layout in ("paired", "bricked")
             for persistent in (True, False)]
GPU_SHARDED_POSES = [0, 2, 4, 7, 9]               # render_sharded: 3 + 2 poses
GPU_N, GPU_R, GPU_S, GPU_ALPHA = 64, 24, 90, 2e-3
GPU_DEADLINE_S = 180


def _gpu_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group(GPU_BACKEND, rank=rank, world_size=world, timeout=INIT_TIMEOUT)
    from diffus_amd import CapturedStep, _lib, render_poses
    from diffus_amd.distributed import allreduce_touched, allreduce_volume_grad, render_sharded
    from diffus_amd.phantom import phantom, pose_ring
    vol = torch.from_numpy(phantom(GPU_N)).cuda()
    src, dirs = pose_ring(GPU_N, 12, GPU_R)
    rec = {}
    for sampler, layout, persistent in GPU_CASES:
        per = None
        for step, g in enumerate(GPU_SCHEDULE[rank]):
            key = f"{sampler}_{layout}_{int(persistent)}_{step}"
            s = torch.from_numpy(src[g]).cuda().contiguous()
            d = torch.from_numpy(dirs[g]).cuda().contiguous()
            own = CapturedStep(vol, s, d, GPU_S, GPU_ALPHA, sampler, layout=layout, persistent=False)
            own.step()                                        # this rank's own gradient, fresh and dense
            st = CapturedStep(vol, s, d, GPU_S, GPU_ALPHA, sampler, layout=layout, persistent=persistent)
            if per is not None:                               # the gradient tensor, scratch and flags live across steps
                st.gvol, st.gvol_k, st.touched = per
            st.zero_grad()                                    # the sequence of bench.py's step_touched
            st.step_mse(_lib.BWD_ALL)
            rec[key + "_pre"] = st.touched.cpu().numpy()
            rec[key + "_moved"] = allreduce_touched(st.gvol_k, st.touched)
            st.finish_grad()
            per = (st.gvol, st.gvol_k, st.touched)
            torch.cuda.synchronize()
            rec[key + "_persistent"] = st.persistent
            rec[key + "_gvol"] = st.gvol.cpu().numpy()
            rec[key + "_own"] = own.gvol.cpu().numpy()
            rec[key + "_flags"] = st.touched.cpu().numpy()
            rec[key + "_scratch_nonzero"] = int((st.gvol_k != 0).sum())
            del own, st
    for sampler in ("trilinear", "nearest"):
        v = vol.clone().requires_grad_(True)
        s = torch.from_numpy(src[GPU_SHARDED_POSES]).cuda()
        d = torch.from_numpy(dirs[GPU_SHARDED_POSES]).cuda()
        _, losses, losses_all = render_sharded(
            lambda v_, s_, d_: render_poses(v_, s_, d_, GPU_S, GPU_ALPHA, sampler=sampler), v, s, d,
            lambda f: (f ** 2).sum((1, 2)))
        losses.sum().backward()
        allreduce_volume_grad(v.grad)
        torch.cuda.synchronize()
        rec[f"sharded_{sampler}_losses"] = losses_all.cpu().numpy()
        rec[f"sharded_{sampler}_gvol"] = v.grad.cpu().numpy()
    np.savez(os.path.join(out_dir, f"g{rank}.npz"), **rec)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_gpu_ranks(tmp_path_factory):
    """Runs the two ranks once for every case (two spawned children, no more); on a failure, or no result within the
    deadline, both are killed and nothing is started again."""
    assert torch.cuda.is_available()
    d = tmp_path_factory.mktemp("gpu_ranks")
    ctx = mp.start_processes(_gpu_worker, args=(2, _free_port(), str(d)), nprocs=2, join=False, start_method="spawn")
    deadline = time.monotonic() + GPU_DEADLINE_S
    try:
        while not ctx.join(timeout=2):
            if time.monotonic() > deadline:
                pytest.fail(f"two GPU ranks: no result within {GPU_DEADLINE_S} s; both killed")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
        for p in ctx.processes:
            p.join(10)
    return [np.load(os.path.join(d, f"g{r}.npz")) for r in range(2)]


_F64 = {}


def _f64_grad(sampler, poses):
    """d/dvolume of sum over `poses` of sum(frame^2), float64 torch autograd over oracle/autograd_ref.py."""
    key = (sampler, tuple(poses))
    if key not in _F64:
        from diffus_amd.phantom import phantom, pose_ring
        from oracle import autograd_ref as ar
        src, dirs = pose_ring(GPU_N, 12, GPU_R)
        v = torch.from_numpy(phantom(GPU_N)).double().requires_grad_(True)
        losses = torch.stack([(ar.render(v, torch.from_numpy(src[p]).double(), torch.from_numpy(dirs[p]).double(), GPU_S,
                                         GPU_ALPHA, 0, sampler, points="f32") ** 2).sum() for p in poses])
        losses.sum().backward()
        _F64[key] = (losses.detach().numpy(), v.grad.numpy())
    return _F64[key]


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,layout,persistent", GPU_CASES)
def test_two_gpu_ranks_allreduce_touched_vs_float64_autograd(two_gpu_ranks, sampler, layout, persistent):
    """Every step of two ranks (real scatter, allreduce_touched, real flush; gradient tensor, scratch and flags carried
    across steps): the handed-back gradient equals float64 autograd of the sum over BOTH ranks' poses (< 1e-3 of the
    max, the same support down to float32 resolution), is the same bits on both ranks, and on every voxel lies within 1e-5 of the max of the sum of the
    two ranks' own single-rank gradients -- so that a lost contribution shows even where it is small; the scratch is
    all-zero and the flags are {0, 2} (PERSISTENT) or 0 (STORE) afterwards."""
    recs = two_gpu_ranks
    worst = dict(f64=0.0, own_sum=0.0, support=0, exempt=0)
    stale_live = 0
    for step in range(len(GPU_SCHEDULE[0])):
        key = f"{sampler}_{layout}_{int(persistent)}_{step}"
        _, ref = _f64_grad(sampler, GPU_SCHEDULE[0][step] + GPU_SCHEDULE[1][step])
        g0, g1 = recs[0][key + "_gvol"], recs[1][key + "_gvol"]
        assert bool(recs[0][key + "_persistent"]) == persistent
        assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32)), (step, "ranks differ")
        own = recs[0][key + "_own"].astype(np.float64) + recs[1][key + "_own"]
        den = float(np.abs(ref).max())
        e64 = float(np.abs(g0 - ref).max()) / den
        e_own = float(np.abs(g0 - own).max()) / float(np.abs(own).max())
        # support: nothing where the float64 gradient is zero (a stale brick's leftover would show here), and a value
        # wherever it is above float32 resolution.  A voxel's gradient is a difference of per-sample terms (dr/dz on both
        # sides of a sample); where they cancel to a few float32 ulps the kernel may return an exact 0 (nearest, pose 6,
        # voxel (49, 45, 32): terms 5.0e-6 that cancel to 8.8e-13, 6.8e-9 of the max), so those voxels are exempt.
        extra = int(((g0 != 0) & (ref == 0)).sum())
        missing = int(((g0 == 0) & (np.abs(ref) > 1e-6 * den)).sum())
        worst = dict(f64=max(worst["f64"], e64 / 1e-3), own_sum=max(worst["own_sum"], e_own / 1e-5),
                     support=max(worst["support"], extra + missing),
                     exempt=max(worst["exempt"], int(((g0 == 0) & (ref != 0)).sum())))
        assert den > 0 and e64 < 1e-3, (step, e64)
        assert e_own <= 1e-5, (step, e_own)
        assert extra == 0 and missing == 0, (step, extra, missing)
        pre0, pre1 = recs[0][key + "_pre"], recs[1][key + "_pre"]
        stale_live += int((((pre0 == 2) & (pre1 == 1)) | ((pre0 == 1) & (pre1 == 2))).sum())
        for r in range(2):
            assert int(recs[r][key + "_scratch_nonzero"]) == 0, (step, r)
            fl = recs[r][key + "_flags"]
            assert set(np.unique(fl).tolist()) <= ({0, 2} if persistent else {0}), (step, r)
            live = (pre0 == 1) | (pre1 == 1)
            assert int(recs[r][key + "_moved"]) == live.size + 128 * int(live.sum()), (step, r)
    if persistent:
        assert stale_live > 0                 # the schedule did make bricks stale on one rank and live on the other
    print(f"\n[two GPU ranks {GPU_BACKEND}] {sampler}/{layout}/persistent={persistent}: worst ratio to the bar: "
          f"f64 {worst['f64']:.3f}, own-sum {worst['own_sum']:.3f}; support mismatches {worst['support']} "
          f"(zeros below float32 resolution: {worst['exempt']}); "
          f"stale-on-one/live-on-other bricks {stale_live}")


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["trilinear", "nearest"])
def test_two_gpu_ranks_render_sharded_vs_float64_autograd(two_gpu_ranks, sampler):
    """render_sharded with the real renderer (diffus_amd.render_poses) and a dense allreduce_volume_grad on two ranks:
    the gathered losses (<= 2e-5 relative) and the summed volume gradient (< 1e-3 of the max) against float64 autograd."""
    ref_l, ref_g = _f64_grad(sampler, GPU_SHARDED_POSES)
    worst_l = worst_g = 0.0
    for r, rec in enumerate(two_gpu_ranks):
        el = float(np.max(np.abs(rec[f"sharded_{sampler}_losses"] - ref_l) / np.abs(ref_l)))
        eg = float(np.abs(rec[f"sharded_{sampler}_gvol"] - ref_g).max() / np.abs(ref_g).max())
        worst_l, worst_g = max(worst_l, el / 2e-5), max(worst_g, eg / 1e-3)
        assert el <= 2e-5, (r, el)
        assert eg < 1e-3, (r, eg)
    assert np.array_equal(two_gpu_ranks[0][f"sharded_{sampler}_gvol"], two_gpu_ranks[1][f"sharded_{sampler}_gvol"])
    print(f"\n[two GPU ranks {GPU_BACKEND}] render_sharded {sampler}: worst ratio to the bar: losses {worst_l:.3f}, "
          f"gradient {worst_g:.3f}")
