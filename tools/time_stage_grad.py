"""Times the stage backward (diffus_trace_rays_bwd, diffus_sample_points_bwd) at config-2 size -- one pose of
pose_ring(256, 32, 256), 256 rays x 512 steps, 256^3 phantom -- for both samplers:
  (a) the composed path forward + backward: trace_rays -> compute_echo_traces -> attenuation -> sum(frame^2) -> backward
      (volume, source and directions require grad);
  (b) render_poses forward + backward on the same pose (the fast path);
  (c) the volume scatter alone: diffus_sample_points_bwd of the nearest-sampler gradient at the pose's 131072 sample
      points into a zeroed canonical gradient, against torch's index_put_(..., accumulate=True) of the same values at
      the same indices (and the trilinear scatter beside it); then the same for the points inside the volume only (more
      than half of the pose's samples lie beyond it and clamp onto border voxels).
Prints one line per timing (mean over N runs after warm-up, CUDA events)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diffus_amd  # noqa: E402
from diffus_amd import _lib  # noqa: E402
from diffus_amd.phantom import phantom, pose_ring  # noqa: E402
from diffus_amd.renderer import _stream  # noqa: E402

N, WARM = 50, 5
S, ALPHA = 512, 1e-4


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3


def main():
    dev = torch.device("cuda", 0)
    vol0 = torch.from_numpy(phantom(256)).to(dev)
    s_all, d_all = pose_ring(256, 32, 256)
    src = torch.from_numpy(s_all[5]).to(dev)
    dirs = torch.from_numpy(d_all[5]).to(dev)
    R = dirs.shape[0]
    att = torch.exp(-ALPHA * torch.arange(S, device=dev).float())[None, :]
    print(f"# tools/time_stage_grad.py on one MI355X: one pose, {R} rays x {S} steps, 256^3 phantom, mean of {N} runs (us)")
    for sampler in ("nearest", "trilinear"):
        V = vol0.clone().requires_grad_(True)
        s = src.clone().requires_grad_(True)
        d = dirs.clone().requires_grad_(True)

        def composed():
            r = diffus_amd.trace_rays(V, s, d, S, sampler, want=("refl",))["refl"]
            e, _ = diffus_amd.compute_echo_traces(r.reshape(R, S - 1))
            torch.autograd.grad(((e * att) ** 2).sum(), (V, s, d))

        def fast():
            f = diffus_amd.render_poses(V, s, d, S, ALPHA, start=0, sampler=sampler)
            torch.autograd.grad((f ** 2).sum(), (V, s, d))

        print(f"(a) {sampler:9s} composed trace_rays -> echo -> attenuation fwd+bwd: {timed(composed):8.1f}")
        print(f"(b) {sampler:9s} render_poses fwd+bwd:                            {timed(fast):8.1f}")

    # (c) the scatter alone, at the pose's sample points
    lib = _lib.load()
    k = torch.arange(S, device=dev, dtype=torch.float32).view(1, S, 1)
    pts = (src.view(1, 1, 3) + k * dirs.unsqueeze(1)).contiguous()
    n = pts.shape[0] * pts.shape[1]
    gvals = torch.randn(n, device=dev)
    x, y, z, _ = diffus_amd.custom_nearest_sampler(vol0, pts, visualize=False)
    idx = (x.reshape(-1), y.reshape(-1), z.reshape(-1))
    gvol = torch.zeros_like(vol0)
    st = _stream(dev)

    def hip_scatter(sm):
        def go():
            _lib.check(lib.diffus_sample_points_bwd(vol0.data_ptr(), 256, 256, 256, _lib.CANONICAL, pts.data_ptr(), n, sm,
                                                    gvals.data_ptr(), gvol.data_ptr(), None, st), "diffus_sample_points_bwd")
        return go

    def torch_scatter():
        gvol.index_put_(idx, gvals, accumulate=True)

    # where the adds land: samples beyond the volume clamp onto its border voxels
    lin = (idx[0] * 256 + idx[1]) * 256 + idx[2]
    counts = torch.bincount(lin, minlength=256 ** 3)
    inside = ((pts.reshape(-1, 3).round() >= 0) & (pts.reshape(-1, 3).round() <= 255)).all(1)
    waves = lin.view(-1, 64)
    print("    %.0f %% of the samples lie beyond the volume and clamp onto border voxels; the busiest voxel takes %.0f %% "
          "of the adds; in %.0f %% of the waves all 64 lanes add to one address"
          % (100 * (1 - float(inside.float().mean())), 100 * float(counts.max()) / n,
             100 * float((waves == waves[:, :1]).all(1).float().mean())))
    pin = pts.reshape(-1, 3)[inside].contiguous()
    gin = gvals[inside].contiguous()
    n_in = pin.shape[0]

    def hip_scatter_inside(sm):
        def go():
            _lib.check(lib.diffus_sample_points_bwd(vol0.data_ptr(), 256, 256, 256, _lib.CANONICAL, pin.data_ptr(), n_in, sm,
                                                    gin.data_ptr(), gvol.data_ptr(), None, st), "diffus_sample_points_bwd")
        return go

    idx_in = tuple(t[inside] for t in idx)

    def torch_scatter_inside():
        gvol.index_put_(idx_in, gin, accumulate=True)

    def zero():
        gvol.zero_()

    print(f"(c) nearest   HIP scatter (diffus_sample_points_bwd), {n} points:   {timed(hip_scatter(_lib.NEAREST)):8.1f}")
    print(f"(c) nearest   torch index_put_(accumulate=True), same points:      {timed(torch_scatter):8.1f}")
    print(f"(c) trilinear HIP scatter (8 corners per point):                   {timed(hip_scatter(_lib.TRILINEAR)):8.1f}")
    print(f"    zeroing the 256^3 canonical gradient (not in the lines above): {timed(zero):8.1f}")
    print(f"(c) nearest   HIP scatter, the {n_in} in-volume points only:        {timed(hip_scatter_inside(_lib.NEAREST)):8.1f}")
    print(f"(c) nearest   torch index_put_, the same in-volume points:         {timed(torch_scatter_inside):8.1f}")
    print(f"(c) trilinear HIP scatter, the in-volume points only:              {timed(hip_scatter_inside(_lib.TRILINEAR)):8.1f}")
    # both scatters add the same values at the same indices: same result up to the float atomic order
    gvol.zero_()
    hip_scatter(_lib.NEAREST)()
    a = gvol.clone()
    gvol.zero_()
    torch_scatter()
    torch.cuda.synchronize()
    print("    max |HIP - index_put_| / max |index_put_| = %.2e" % float((a - gvol).abs().max() / gvol.abs().max()))


if __name__ == "__main__":
    main()
