"""Linear and convex array probes on the GPU: one beam origin per ray (DIFFUS_SRC_PER_RAY).

The reference evaluates source + k * dir for one source per pose (src/renderer.py:119-124).  Per-ray sources apply that
formula row by row, so row r of a per-ray frame is the oracle's one-ray frame of (src[r], dirs[r]); with start > 0 the
median of the first kept coefficient is taken across the pose's rays, as for a fan.  Gradients are held against float64
autograd through oracle/autograd_ref.py at the float32 sample points, the bars of the fan tests.
"""
import numpy as np
import pytest
import torch

from conftest import maxnorm_rel
from diffus_amd.phantom import phantom

pytestmark = pytest.mark.gpu

N = 64


@pytest.fixture(scope="module")
def da():
    import diffus_amd
    from diffus_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return diffus_amd


@pytest.fixture(scope="module")
def vol():
    return phantom(N)


@pytest.fixture(scope="module")
def smooth():
    u = np.arange(N, dtype=np.float64) / (N - 1)
    v = 1.6e6 + 3e5 * np.sin(6 * u)[:, None, None] * np.cos(5 * u)[None, :, None] * np.sin(4 * u + 1)[None, None, :]
    return v.astype(np.float32)


def arrays(kind, R, dtype=np.float32, seed=0):
    """(src (R,3), dirs (R,3)) of one probe in the 64^3 head."""
    import diffus_amd as da
    if kind == "linear":
        s, d = da.linear_array(torch.tensor([8.0, 32.0, 31.3], dtype=torch.float64), [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], R, 30.0)
    elif kind == "tilted":
        s, d = da.linear_array(torch.tensor([8.0, 32.0, 30.0], dtype=torch.float64), [1.0, 0.05, 0.2], [0.0, 1.0, 0.3], R, 30.0)
    elif kind == "convex":
        s, d = da.convex_array(torch.tensor([-4.0, 32.0, 29.6], dtype=torch.float64), [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], 10.0, 1.0, R)
    elif kind == "random":       # origins outside the volume on every side: the clamp path
        rng = np.random.default_rng(seed)
        s = rng.uniform(-20.0, 84.0, (R, 3))
        s[:, 0] = np.where(rng.random(R) < 0.5, -15.0, 80.0)
        d = 32.0 - s + rng.normal(0, 6.0, (R, 3))
        s, d = torch.from_numpy(s), torch.from_numpy(d / np.linalg.norm(d, axis=1, keepdims=True))
    elif kind == "heights":      # dim-2 directions of 0, origins at different dim-2 heights
        s, d = da.linear_array(torch.tensor([8.0, 32.0, 30.0], dtype=torch.float64), [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], R, 30.0)
        s = s.clone()
        s[:, 2] = 30.0 + 4.0 * torch.linspace(-1.0, 1.0, R, dtype=torch.float64) ** 2
    s, d = s.numpy().astype(dtype), d.numpy().astype(np.float32)
    d[np.abs(d) < 1e-12] = 0.0
    return np.ascontiguousarray(s), np.ascontiguousarray(d)


def oracle_rows(v, src, dirs, S, alpha, sampler):
    """Oracle frame row by row, start = 0: (x, y, z, frame) stacked over rays, and per ray the float64 frame and its
    conditioning tolerance (oracle/conditioning.py)."""
    from oracle import oracle as orc
    from oracle.conditioning import frame64_and_tolerance
    out = [orc.plot_beam_frame(v, src[r], dirs[r:r + 1], S, alpha, 0, sampler=sampler) for r in range(len(src))]
    xyz_f = [np.concatenate([o[i] for o in out]) for i in range(4)]
    tols = [frame64_and_tolerance(v, src[r], dirs[r:r + 1], S, alpha, sampler=sampler) for r in range(len(src))]
    return xyz_f, tols


def check_frame(f, xyz_f, tols, idx=None):
    fo = xyz_f[3]
    den = np.abs(fo).max()
    for r in range(len(fo)):
        f64, tol, _ = tols[r]
        err = np.abs(f[r].astype(np.float64) - f64[0]).max()
        assert err <= max(2e-5 * den, tol * np.abs(f64).max()) or np.abs(f[r] - fo[r]).max() <= 2e-5 * den, (r, err, den, tol)
    if idx is not None:
        for c in range(3):
            np.testing.assert_array_equal(idx[c], xyz_f[c])


@pytest.mark.parametrize("layout", ["canonical", "bricked", "paired"])
@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
@pytest.mark.parametrize("sdt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["linear", "convex", "random"])
def test_per_ray_frame_rows_equal_one_ray_oracle_frames(da, vol, kind, sdt, sampler, layout):
    R, S, alpha = 24, 160, 2e-3
    src, dirs = arrays(kind, R, sdt)
    xyz_f, tols = oracle_rows(vol, src, dirs, S, alpha, sampler)
    v = torch.from_numpy(vol).cuda()
    f, idx = da.render_poses(v, torch.from_numpy(src).cuda()[None], torch.from_numpy(dirs).cuda(), S, alpha, sampler=sampler,
                             return_indices=True, layout=layout)
    assert f.shape == (1, R, S) and idx.shape == (3, 1, R, S)
    check_frame(f[0].cpu().numpy(), xyz_f, tols, idx[:, 0].cpu().numpy())


def composed_frame(v, src, dirs, S, alpha, start, sampler):
    """Per-ray sample_*, then reflection, start_crop (the median across the rays), echo_scan, attenuate (oracle)."""
    from oracle import oracle as orc
    if sampler == "trilinear":
        imp = np.concatenate([orc.sample_trilinear(v, src[r], dirs[r:r + 1], S) for r in range(len(src))])
    else:
        imp = np.concatenate([orc.sample_nearest(v, src[r], dirs[r:r + 1], S)[3] for r in range(len(src))])
    r, _, _ = orc.start_crop(orc.reflection(imp), start)
    return orc.attenuate(orc.echo_scan(r), alpha)


@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
@pytest.mark.parametrize("kind", ["linear", "convex", "tilted"])
def test_per_ray_frame_with_start_matches_the_composition(da, smooth, kind, sampler):
    R, S, alpha, start = 21, 140, 2e-3, 9
    src, dirs = arrays(kind, R)
    fo = composed_frame(smooth, src, dirs, S, alpha, start, sampler)
    for layout in ("canonical", "paired"):
        f = da.render_poses(torch.from_numpy(smooth).cuda(), torch.from_numpy(src).cuda()[None], torch.from_numpy(dirs).cuda(),
                            S, alpha, start=start, sampler=sampler, layout=layout)
        assert maxnorm_rel(f[0].cpu().numpy(), fo) <= 2e-5, layout


@pytest.mark.parametrize("S", [1500, 3000])
@pytest.mark.parametrize("kind", ["linear", "convex"])
def test_per_ray_long_rays(da, vol, kind, S):
    """Rays of more than 1024 samples: chained segments and the float64 long-ray repair read each ray's own source."""
    R, alpha = 8, 1e-4
    src, dirs = arrays(kind, R)
    dirs = np.ascontiguousarray(dirs * np.float32(60.0 / S))
    xyz_f, tols = oracle_rows(vol, src, dirs, S, alpha, "trilinear")
    f = da.render_poses(torch.from_numpy(vol).cuda(), torch.from_numpy(src).cuda()[None], torch.from_numpy(dirs).cuda(), S,
                        alpha, sampler="trilinear")
    check_frame(f[0].cpu().numpy(), xyz_f, tols)


@pytest.mark.parametrize("start", [0, 7])
@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
def test_equal_per_ray_sources_reproduce_the_shared_source_call(da, vol, sampler, start):
    from diffus_amd.phantom import pose_ring
    P, R, S, alpha = 3, 40, 200, 2e-3
    src, dirs = pose_ring(N, P, R)
    v = torch.from_numpy(vol).cuda()
    out = []
    for s in (torch.from_numpy(src).cuda(), torch.from_numpy(src).cuda()[:, None, :].expand(P, R, 3).contiguous()):
        vv = v.clone().requires_grad_(True)
        s = s.clone().requires_grad_(True)
        d = torch.from_numpy(dirs).cuda().requires_grad_(True)
        f = da.render_poses(vv, s, d, S, alpha, start=start, sampler=sampler)
        w = torch.randn(f.shape, generator=torch.Generator().manual_seed(3)).cuda()
        (f * w).sum().backward()
        out.append((f.detach(), vv.grad, s.grad, d.grad))
    (f1, gv1, gs1, gd1), (f2, gv2, gs2, gd2) = out
    assert gs2.shape == (P, R, 3)
    assert torch.equal(f1, f2)
    assert torch.equal(gd1, gd2)
    assert (gs2.sum(1) - gs1).abs().max() <= 1e-6 * max(gs1.abs().max().item(), 1e-30) or sampler == "nearest" and gs2.abs().max() == 0
    assert maxnorm_rel(gv2.cpu().numpy(), gv1.cpu().numpy()) < 1e-5


def autograd_reference(v, src, dirs, S, alpha, start, w):
    """float64 autograd through the oracle's restatement, per-ray sample points at float32 rounding."""
    from oracle import autograd_ref as ar
    v64 = torch.from_numpy(v).double().requires_grad_(True)
    s64 = torch.from_numpy(src).double().requires_grad_(True)
    d64 = torch.from_numpy(dirs).double().requires_grad_(True)
    R = src.shape[0]
    pts = torch.cat([ar.ray_points_f32(s64[r], d64[r:r + 1], S) for r in range(R)])
    r = ar.start_crop(ar.reflection(ar.sample_trilinear(v64, pts)), start)
    echo = ar.echo_scan(r)
    f = echo * torch.exp(-alpha * torch.arange(echo.shape[1], dtype=torch.float64))[None, :]
    (f * w.double()).sum().backward()
    return f.detach().numpy(), v64.grad.numpy(), s64.grad.numpy(), d64.grad.numpy()


@pytest.mark.parametrize("start", [0, 6])
@pytest.mark.parametrize("kind", ["linear", "tilted", "convex", "heights"])
def test_per_ray_gradients_vs_float64_autograd(da, smooth, kind, start):
    R, S, alpha = 20, 120, 3e-3
    src, dirs = arrays(kind, R)
    w = torch.randn((R, S - start), generator=torch.Generator().manual_seed(7))
    f_ref, gv_ref, gs_ref, gd_ref = autograd_reference(smooth, src, dirs, S, alpha, start, w)
    for layout in ("canonical", "bricked", "paired"):
        v = torch.from_numpy(smooth).cuda().requires_grad_(True)
        s = torch.from_numpy(src).cuda()[None].requires_grad_(True)
        d = torch.from_numpy(dirs).cuda()[None].requires_grad_(True)
        f = da.render_poses(v, s, d, S, alpha, start=start, sampler="trilinear", layout=layout)
        assert maxnorm_rel(f[0].detach().cpu().numpy(), f_ref) < 2e-5
        (f[0] * w.cuda()).sum().backward()
        assert s.grad.shape == (1, R, 3)
        assert maxnorm_rel(v.grad.cpu().numpy(), gv_ref) < 1e-3, layout
        assert maxnorm_rel(s.grad[0].cpu().numpy(), gs_ref) < 1e-3, layout
        assert maxnorm_rel(d.grad[0].cpu().numpy(), gd_ref) < 1e-3, layout


@pytest.mark.parametrize("start", [0, 5])
@pytest.mark.parametrize("kind", ["linear", "tilted"])
def test_captured_step_with_per_ray_sources_equals_the_two_call_path(da, smooth, kind, start):
    P, R, S, alpha = 2, 32, 128, 2e-3
    s0, d0 = arrays(kind, R)
    src = np.stack([s0, s0 + np.float32([1.0, 2.0, 0.0])])
    dirs = np.stack([d0, d0])
    v = torch.from_numpy(smooth).cuda()
    tgt = torch.zeros((P, R, S - start), device="cuda")
    step = da.CapturedStep(v, torch.from_numpy(src).cuda(), torch.from_numpy(dirs).cuda(), S, alpha, "trilinear", start=start,
                           target=tgt)
    assert step.gsrc.shape == (P, R, 3)

    def two_call(s, d):
        vv = v.clone().requires_grad_(True)
        ss = s.clone().requires_grad_(True)
        dd = d.clone().requires_grad_(True)
        f = da.render_poses(vv, ss, dd, S, alpha, start=start, sampler="trilinear", layout="paired")
        ((f - tgt) ** 2).sum(dim=(1, 2)).sum().backward()
        return f.detach(), vv.grad, ss.grad, dd.grad

    def check(s, d):
        f, gv, gs, gd = two_call(s, d)
        assert maxnorm_rel(step.frame.cpu().numpy(), f.cpu().numpy()) < 2e-5
        assert maxnorm_rel(step.gvol.cpu().numpy(), gv.cpu().numpy()) < 1e-4
        assert maxnorm_rel(step.gsrc.cpu().numpy(), gs.cpu().numpy()) < 1e-4
        assert maxnorm_rel(step.gdirs.cpu().numpy(), gd.cpu().numpy()) < 1e-4

    step.step()
    torch.cuda.synchronize()
    check(torch.from_numpy(src).cuda(), torch.from_numpy(dirs).cuda())
    step.capture()
    src2 = torch.from_numpy(src + np.float32([0.5, -1.0, 0.0])).cuda()
    step.set_poses(src2)
    step.replay()
    torch.cuda.synchronize()
    check(src2, torch.from_numpy(dirs).cuda())
    # render() / mse_loss(): the autograd nodes hand back (P,R,3) source gradients
    s = src2.clone().requires_grad_(True)
    loss = step.mse_loss(None, s, None)
    loss.backward()
    assert s.grad.shape == (P, R, 3)
    f = step.render(None, src2, None)
    assert f.shape == (P, R, S - start)


@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
def test_trace_rays_per_ray_forward_and_backward(da, smooth, sampler):
    from oracle import autograd_ref as ar
    from oracle import oracle as orc
    R, S = 16, 90
    src, dirs = arrays("convex", R)
    v = torch.from_numpy(smooth).cuda().requires_grad_(True)
    s = torch.from_numpy(src).cuda()[None].requires_grad_(True)
    d = torch.from_numpy(dirs).cuda().requires_grad_(True)
    out = da.trace_rays(v, s, d, S, sampler=sampler)
    if sampler == "trilinear":
        imp_o = np.concatenate([orc.sample_trilinear(smooth, src[r], dirs[r:r + 1], S) for r in range(R)])
    else:
        imp_o = np.concatenate([orc.sample_nearest(smooth, src[r], dirs[r:r + 1], S)[3] for r in range(R)])
    np.testing.assert_array_equal(out["imp"][0].detach().cpu().numpy(), imp_o)
    np.testing.assert_array_equal(out["refl"][0].detach().cpu().numpy(), orc.reflection(imp_o))
    gi = torch.randn(out["imp"].shape, generator=torch.Generator().manual_seed(1)).cuda()
    gr = torch.randn(out["refl"].shape, generator=torch.Generator().manual_seed(2)).cuda()
    ((out["imp"] * gi).sum() + (out["refl"] * gr).sum()).backward()
    assert s.grad.shape == (1, R, 3)
    v64 = torch.from_numpy(smooth).double().requires_grad_(True)
    s64 = torch.from_numpy(src).double().requires_grad_(True)
    d64 = torch.from_numpy(dirs).double().requires_grad_(True)
    pts = torch.cat([ar.ray_points_f32(s64[r], d64[r:r + 1], S) for r in range(R)])
    imp = ar.sample_trilinear(v64, pts) if sampler == "trilinear" else ar.sample_nearest(v64, pts)[0]
    ((imp * gi.cpu().double()[0]).sum() + (ar.reflection(imp) * gr.cpu().double()[0]).sum()).backward()
    assert maxnorm_rel(v.grad.cpu().numpy(), v64.grad.numpy()) < 1e-3
    if sampler == "trilinear":
        assert maxnorm_rel(s.grad[0].cpu().numpy(), s64.grad.numpy()) < 1e-3
        assert maxnorm_rel(d.grad.cpu().numpy(), d64.grad.numpy()) < 1e-3
    else:
        assert torch.all(s.grad == 0)


def test_array_pose_registration_through_the_hip_backward(da, smooth):
    """ArrayPose recovers a 3 degree tilt plus a 2-voxel offset of a linear array (mirrors
    test_pose_sweep_registration_batched)."""
    R, S, alpha = 32, 96, 1e-3
    c = torch.tensor([10.0, 32.0, 31.3])
    src, dirs = da.linear_array(c, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], R, 28.0)
    vol = torch.from_numpy(smooth).cuda()
    true = da.ArrayPose(c, src - c, dirs, rotvec=torch.zeros(3)).cuda()
    with torch.no_grad():
        target = da.render_poses(vol, *true(), S, alpha, sampler="trilinear")
    tilt = np.deg2rad(3.0)
    pose = da.ArrayPose(c + torch.tensor([2.0, 0.0, 0.0]), src - c, dirs, rotvec=torch.tensor([0.0, tilt, 0.0])).cuda()
    opt = torch.optim.Adam([{"params": [pose.origin], "lr": 0.05}, {"params": [pose.rotvec], "lr": 0.004}])
    first = last = None
    for it in range(200):
        opt.zero_grad()
        f = da.render_poses(vol, *pose(), S, alpha, sampler="trilinear")
        loss = ((f - target) ** 2).sum()
        loss.backward()
        opt.step()
        if it == 0:
            first = loss.item()
        last = loss.item()
    assert last < 0.1 * first, (first, last)

