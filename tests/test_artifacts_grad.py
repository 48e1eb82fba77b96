"""Gradient of the artifact chain (plot_beam_frame(artifacts=True), apply_artifacts; diffus_artifacts_bwd).

"Correct" is the gradient torch autograd gives for the chain restated in float64 torch ops below:
speckle `s[s < 0] = 0`, the two 'reflect' Gaussian filters as gathers, and the clip as
torch.clamp(u, x.amin(), x.amax()) per frame (a bound's gradient shared evenly among its ties).
The restatement is pinned to the oracle (and so to golden G14) on the CPU first."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, maxnorm_rel


# ---------------------------------------------------------------- float64 torch restatement (test only)
def _reflect(j, n):
    j = np.mod(j, 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def _taps(sigma):
    """oracle.artifacts.gaussian_filter1d's normalised kernel; None for the identity (radius 0)."""
    rad = int(4.0 * sigma + 0.5)
    if rad == 0:
        return None
    x = np.arange(-rad, rad + 1)
    k = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return k / k.sum()


def _filter(a, sigma, axis):
    k = _taps(sigma)
    if k is None:
        return a
    rad = (len(k) - 1) // 2
    n = a.shape[axis]
    out = torch.zeros_like(a)
    for t, w in zip(range(-rad, rad + 1), k):
        out = out + float(w) * a.index_select(axis, torch.from_numpy(_reflect(np.arange(n) + t, n)))
    return out


def _lateral_blur(s, max_sigma):
    """per column z: sigma_z = max_sigma z/(N-1) (1e-8 at z = 0) along the rays; tap t of every column in one op
    (a zero weight beyond a column's radius adds exact zeros: the oracle's order of summation is kept)."""
    R, N = s.shape
    ks = [_taps(max_sigma * (z / (N - 1)) if z > 0 else 1e-8) for z in range(N)]
    ks = [np.ones(1) if k is None else k for k in ks]
    rmax = max((len(k) - 1) // 2 for k in ks)
    W = np.zeros((2 * rmax + 1, N))
    for z, k in enumerate(ks):
        r = (len(k) - 1) // 2
        W[rmax - r:rmax + r + 1, z] = k
    out = torch.zeros_like(s)
    for t in range(-rmax, rmax + 1):
        out = out + torch.from_numpy(W[t + rmax])[None, :] * s[torch.from_numpy(_reflect(np.arange(R) + t, R))]
    return out


def restated(frame, std_radial, std_local, max_sigma, alpha, radial, local, parts=False):
    """One frame (R,N) float64 tensor -> the chain's output; `parts`: also the intermediates for branch checks."""
    noised = frame * (radial[None, :] * local)
    s = noised.clone()
    s[s < 0] = 0.0
    x = _lateral_blur(s, max_sigma)
    u = x + alpha * (x - _filter(_filter(x, 1.0, 0), 1.0, 1))
    lo, hi = x.amin(), x.amax()
    y = torch.clamp(u, lo, hi)
    if parts:
        return y, dict(noised=noised, x=x, u=u, lo=lo, hi=hi)
    return y


def restated_grad(frames, gy, params, radial, local):
    """d sum(y * gy) / d frames for frames (P,R,N) float64 numpy, noise (P,N), (P,R,N) -> (P,R,N) numpy, and branch
    counts over all frames."""
    f = torch.from_numpy(np.asarray(frames, np.float64)).requires_grad_(True)
    hits = dict(clip_lo=0, clip_hi=0, ties_lo=0, ties_hi=0, masked=0)
    ys = []
    for p in range(f.shape[0]):
        y, pt = restated(f[p], *params, torch.from_numpy(np.asarray(radial[p])), torch.from_numpy(np.asarray(local[p])),
                         parts=True)
        ys.append(y)
        hits["clip_lo"] += int((pt["u"] < pt["lo"]).sum())
        hits["clip_hi"] += int((pt["u"] > pt["hi"]).sum())
        hits["ties_lo"] = max(hits["ties_lo"], int((pt["x"] == pt["lo"]).sum()))
        hits["ties_hi"] = max(hits["ties_hi"], int((pt["x"] == pt["hi"]).sum()))
        hits["masked"] += int((pt["noised"] < 0).sum())
    (g,) = torch.autograd.grad(torch.stack(ys), f, torch.from_numpy(np.asarray(gy, np.float64)))
    return g.numpy(), np.stack([y.detach().numpy() for y in ys]), hits


# ---------------------------------------------------------------- CPU
def test_restatement_matches_oracle_on_g14():
    from oracle import artifacts as oa
    g = load_golden("g14_artifacts")
    for t in [str(t) for t in g["tags"]]:
        sr, sl, ms, al = (float(v) for v in g[f"{t}_params"])
        fr, rad, loc = g[f"{t}_frame"], g[f"{t}_radial"], g[f"{t}_local"]
        ref = oa.chain(fr, sr, sl, ms, al, rad, loc)
        got = restated(torch.from_numpy(np.asarray(fr, np.float64)), sr, sl, ms, al, torch.from_numpy(rad),
                       torch.from_numpy(loc)).numpy()
        assert maxnorm_rel(got, ref) <= 1e-13, t


@pytest.mark.parametrize("R,N,max_sigma", [(6, 5, 2.0), (9, 12, 0.7), (1, 4, 1.5)])
def test_restatement_gradcheck(R, N, max_sigma):
    """small tie-free inputs: positive frame and noise (nothing masked), distinct values (unique min and max)"""
    rng = np.random.default_rng(R * 100 + N)
    f = torch.from_numpy(rng.uniform(0.5, 2.0, size=(R, N))).requires_grad_(True)
    radial = torch.from_numpy(rng.uniform(0.9, 1.1, size=N))
    local = torch.from_numpy(rng.uniform(0.8, 1.2, size=(R, N)))
    assert torch.autograd.gradcheck(lambda a: restated(a, 0.05, 0.1, max_sigma, 2.5, radial, local), (f,),
                                    eps=1e-6, atol=1e-8, rtol=1e-6)


@pytest.fixture(scope="module")
def lib():
    from diffus_amd import build, _lib
    build.build()
    return _lib.load()


def test_backward_entry_points_exported_and_cite_the_reference(lib):
    import os
    from diffus_amd import _lib
    for n in ("diffus_artifacts_bwd_workspace_bytes", "diffus_artifacts_bwd", "diffus_artifacts_noise"):
        assert n in _lib.EXPORTS and getattr(lib, n) is not None
    assert lib.diffus_abi_version() == 8
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffus_hip.h")).read()
    for fn in ("diffus_artifacts_bwd", "diffus_artifacts_noise"):
        i = txt.index("int " + fn + "(")
        assert "src/renderer.py:535-601" in txt[txt.rfind("/*", 0, i): i], fn


def test_backward_argument_validation_without_a_gpu(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.diffus_artifacts_bwd_workspace_bytes(0, 4, 4) == 0
    assert lib.diffus_artifacts_bwd_workspace_bytes(2, 4, -1) == 0
    wsb = lib.diffus_artifacts_bwd_workspace_bytes(32, 256, 512)
    assert wsb >= lib.diffus_artifacts_workspace_bytes(32, 256, 512) and wsb % 256 == 0
    ok = dict(frame=p, P=1, R=2, N=3, sr=0.01, sl=0.15, ms=4.0, al=5.0, rad=None, loc=None, seed=1, gout=p, gframe=p,
              ws=p, wsb=wsb)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.diffus_artifacts_bwd(a["frame"], a["P"], a["R"], a["N"], a["sr"], a["sl"], a["ms"], a["al"], a["rad"],
                                        a["loc"], a["seed"], a["gout"], a["gframe"], a["ws"], a["wsb"], None)

    assert bwd(frame=None) == -1
    assert bwd(gout=None) == -1
    assert bwd(gframe=None) == -1
    assert bwd(P=0) == -1
    assert bwd(R=-3) == -1
    assert bwd(N=0) == -1
    assert bwd(ms=-1.0) == -1
    assert bwd(ms=float("nan")) == -1
    assert bwd(sr=-0.1) == -1
    assert bwd(ws=None) == -4
    assert bwd(wsb=lib.diffus_artifacts_bwd_workspace_bytes(1, 2, 3) - 1) == -4
    assert lib.diffus_artifacts_noise(1, 2, 3, 0.01, 0.15, 7, None, p, None) == -1
    assert lib.diffus_artifacts_noise(1, 2, 3, 0.01, 0.15, 7, p, None, None) == -1
    assert lib.diffus_artifacts_noise(0, 2, 3, 0.01, 0.15, 7, p, p, None) == -1
    assert lib.diffus_artifacts_noise(1, 2, 3, -1.0, 0.15, 7, p, p, None) == -1


# ---------------------------------------------------------------- GPU
def _gpu_grad(frames, gy, params, noise=None, seed=None):
    import diffus_amd
    f = torch.from_numpy(np.asarray(frames, np.float64)).cuda().requires_grad_(True)
    out = diffus_amd.apply_artifacts(f, *params, seed=seed, noise=noise)
    (g,) = torch.autograd.grad(out, f, torch.from_numpy(np.asarray(gy, np.float64)).cuda())
    return out.detach().cpu().numpy(), g.cpu().numpy()


def _f32(a):
    """float64 values a float32 frame holds exactly: the restatement and the kernels then see the same frame"""
    return np.asarray(a, np.float32).astype(np.float64)


@pytest.mark.gpu
def test_apply_artifacts_records_a_backward():
    import diffus_amd
    f = torch.rand((2, 16, 40), device="cuda").requires_grad_(True)
    out = diffus_amd.apply_artifacts(f, seed=1)
    assert out.grad_fn is not None and out.dtype == torch.float64 and out.shape == f.shape
    out.sum().backward()
    assert f.grad is not None and f.grad.dtype == torch.float32 and f.grad.shape == f.shape
    assert torch.isfinite(f.grad).all() and f.grad.abs().sum() > 0
    f2 = torch.rand((16, 40), device="cuda", dtype=torch.float64).requires_grad_(True)       # 2-D, float64
    (g2,) = torch.autograd.grad(diffus_amd.apply_artifacts(f2, seed=2).sum(), f2)
    assert g2.shape == f2.shape and g2.dtype == torch.float64 and g2.device == f2.device
    with torch.no_grad():
        assert diffus_amd.apply_artifacts(f, seed=1).grad_fn is None
    fc = f.detach().cpu().requires_grad_(True)                                               # host frame: host gradient
    (gc,) = torch.autograd.grad(diffus_amd.apply_artifacts(fc, seed=1).sum(), fc)
    assert gc.device.type == "cpu" and torch.equal(gc, f.grad.cpu())


@pytest.mark.gpu
def test_grad_matches_restatement_g14_injected_noise():
    g = load_golden("g14_artifacts")
    rng = np.random.default_rng(14)
    for t in [str(t) for t in g["tags"]]:
        params = tuple(float(v) for v in g[f"{t}_params"])
        fr = _f32(g[f"{t}_frame"])[None]
        rad, loc = g[f"{t}_radial"][None], g[f"{t}_local"][None]
        gy = rng.normal(size=fr.shape)
        ref, yref, _ = restated_grad(fr, gy, params, rad, loc)
        y, got = _gpu_grad(fr, gy, params, noise=(rad, loc))
        assert maxnorm_rel(y, yref) < 1e-12, t
        assert maxnorm_rel(got, ref) <= 1e-10, t


@pytest.mark.gpu
def test_seeded_noise_companion_and_seeded_grad():
    import diffus_amd
    rng = np.random.default_rng(5)
    P, R, N = 2, 48, 90
    params = (0.05, 0.2, 3.0, 4.0)
    fr = _f32(rng.normal(0.2, 1.0, size=(P, R, N)))
    fc = torch.from_numpy(fr).float().cuda()
    radial, local = diffus_amd.artifact_noise((P, R, N), 0.05, 0.2, seed=11)
    assert radial.shape == (P, N) and local.shape == (P, R, N) and radial.dtype == torch.float64
    seeded = diffus_amd.apply_artifacts(fc, *params, seed=11)
    assert torch.equal(seeded, diffus_amd.apply_artifacts(fc, *params, noise=(radial, local)))     # bitwise
    r1, l1 = diffus_amd.artifact_noise((R, N), 0.05, 0.2, seed=11)                              # one frame: pose 0
    assert torch.equal(r1, radial[0]) and torch.equal(l1, local[0])
    assert torch.equal(diffus_amd.apply_artifacts(fc[0], *params, seed=11), seeded[0])
    gy = rng.normal(size=(P, R, N))
    ref, yref, hits = restated_grad(fr, gy, params, radial.cpu().numpy(), local.cpu().numpy())
    y, got = _gpu_grad(fr, gy, params, seed=11)
    assert maxnorm_rel(y, yref) < 1e-12
    assert maxnorm_rel(got, ref) <= 1e-10
    assert hits["masked"] > 0
    # auto-seeded: the backward goes through the draws the forward made
    f = torch.from_numpy(fr).cuda().requires_grad_(True)
    out = diffus_amd.apply_artifacts(f, *params)
    (ga,) = torch.autograd.grad(out, f, torch.from_numpy(gy).cuda())
    seed = out.grad_fn.launch[4]
    r2, l2 = diffus_amd.artifact_noise((P, R, N), 0.05, 0.2, seed=seed)
    assert torch.equal(out.detach(), diffus_amd.apply_artifacts(fc, *params, noise=(r2, l2)))
    ref2, _, _ = restated_grad(fr, gy, params, r2.cpu().numpy(), l2.cpu().numpy())
    assert maxnorm_rel(ga.cpu().numpy(), ref2) <= 1e-10


def _noise(rng, P, R, N, sr, sl):
    from oracle import artifacts as oa
    rs, ls = oa.noise_scales(N, sr, sl)
    return rng.normal(1.0, rs, size=(P, N)), rng.normal(1.0, ls[None, None, :], size=(P, R, N))


@pytest.mark.gpu
@pytest.mark.parametrize("R,N,max_sigma", [(40, 70, 3.0), (37, 150, 7.6), (90, 65, 12.0), (5, 33, 4.0), (300, 700, 4.0),
                                           (1, 40, 4.0), (30, 2, 4.0)])
@pytest.mark.parametrize("alpha", [0.0, 5.0])
def test_grad_shapes_radii_alpha(R, N, max_sigma, alpha):
    """tile borders, rays fewer than the blur radius (repeated reflection), both blur paths (weights in LDS up to
    radius 30, the direct form beyond), R = 1 and N = 2; signed frames, so the speckle masks and the minimum is tied"""
    rng = np.random.default_rng(R * 1000 + N)
    params = (0.05, 0.1, max_sigma, alpha)
    fr = _f32(rng.normal(0.3, 1.0, size=(2, R, N)))
    radial, local = _noise(rng, 2, R, N, 0.05, 0.1)
    gy = rng.normal(size=fr.shape)
    ref, yref, hits = restated_grad(fr, gy, params, radial, local)
    y, got = _gpu_grad(fr, gy, params, noise=(radial, local))
    assert maxnorm_rel(y, yref) < 1e-12
    assert maxnorm_rel(got, ref) <= 1e-10, (R, N, max_sigma, alpha)
    assert hits["masked"] > 0


def _tied_case(rng, P=2, R=64, N=96):
    """exact ties at the min (zero plateau the speckle leaves, wider than the blur) and at the max (equal spikes in
    column 0, whose blur is the identity), elements clipped on both sides"""
    fr = rng.normal(0.5, 1.0, size=(P, R, N))
    fr[:, 20:45, :] = -1.0                      # masked by the speckle -> x == 0 == min over a block of rays
    fr[:, [3, 9, 50, 60], 0] = 40.0             # the max, reached four times per frame
    radial, local = _noise(rng, P, R, N, 0.05, 0.1)
    radial[:, 0] = 1.0
    local[:, [3, 9, 50, 60], 0] = 1.0
    return _f32(fr), radial, local


@pytest.mark.gpu
def test_grad_exact_ties_and_clipping_both_sides():
    rng = np.random.default_rng(77)
    fr, radial, local = _tied_case(rng)
    for params in ((0.05, 0.1, 4.0, 5.0), (0.05, 0.1, 9.0, 2.0)):
        gy = rng.normal(size=fr.shape)
        ref, yref, hits = restated_grad(fr, gy, params, radial, local)
        assert hits["clip_lo"] > 0 and hits["clip_hi"] > 0 and hits["masked"] > 0
        assert hits["ties_lo"] > 1 and hits["ties_hi"] == 4
        y, got = _gpu_grad(fr, gy, params, noise=(radial, local))
        assert maxnorm_rel(y, yref) < 1e-12
        assert maxnorm_rel(got, ref) <= 1e-10, params


@pytest.mark.gpu
def test_backward_bitwise_repeatable_and_forward_unchanged_by_grad():
    import diffus_amd
    rng = np.random.default_rng(3)
    fr, radial, local = _tied_case(rng, P=4, R=256, N=300)
    f = torch.from_numpy(fr).float().cuda()
    gy = torch.from_numpy(rng.normal(size=fr.shape)).cuda()
    for kw in (dict(seed=9), dict(noise=(radial, local))):
        off = diffus_amd.apply_artifacts(f, **kw)
        fg = f.clone().requires_grad_(True)
        on = diffus_amd.apply_artifacts(fg, **kw)
        assert torch.equal(off, on.detach())
        (g1,) = torch.autograd.grad(on, fg, gy, retain_graph=True)
        (g2,) = torch.autograd.grad(on, fg, gy)
        assert torch.equal(g1, g2)


@pytest.mark.gpu
def test_backward_refuses_frames_modified_in_place():
    import diffus_amd
    f = torch.rand((8, 20), device="cuda").requires_grad_(True)
    a = f * 1.0
    out = diffus_amd.apply_artifacts(a, seed=1)
    with torch.no_grad():
        a.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        out.sum().backward()


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
def test_plot_beam_frame_artifacts_backward(sampler):
    import diffus_amd
    from diffus_amd.phantom import phantom, pose_ring
    vol0 = torch.from_numpy(phantom(64)).cuda()
    s, d = pose_ring(64, 2, 32)
    src0, dirs0 = torch.from_numpy(s[0]).cuda(), torch.from_numpy(d[0]).cuda()
    Rr = diffus_amd.UltrasoundRenderer(80, 1e-3)
    params = dict(std_radial=0.01, std_local=0.15, max_sigma=4.0, alpha=5)
    tri = sampler == "trilinear"

    def leaves():
        v = vol0.clone().requires_grad_(True)
        sr = src0.clone().requires_grad_(tri)
        dr = dirs0.clone().requires_grad_(tri)
        return v, sr, dr

    v, sr, dr = leaves()
    _, _, _, frame = Rr.plot_beam_frame(v, sr, dr, artifacts=True, start=10, seed=4, sampler=sampler, **params)
    assert frame.dtype == torch.float64 and frame.shape == (32, 70) and frame.grad_fn is not None
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.normal(size=(32, 70))).cuda()
    (frame * w).sum().backward()
    # the same through render_poses autograd fed with the restatement's frame gradient
    v2, s2, d2 = leaves()
    rf = diffus_amd.render_poses(v2, s2, d2, 80, 1e-3, start=10, sampler=sampler)[0]
    radial, local = diffus_amd.artifact_noise(rf.shape, params["std_radial"], params["std_local"], seed=4)
    gref, yref, _ = restated_grad(rf.detach().double().cpu().numpy()[None], w.cpu().numpy()[None],
                                  tuple(params.values()), radial.cpu().numpy()[None], local.cpu().numpy()[None])
    assert maxnorm_rel(frame.detach().cpu().numpy(), yref[0]) < 1e-12
    ins = (v2, s2, d2) if tri else (v2,)
    refs = torch.autograd.grad(rf, ins, torch.from_numpy(gref[0]).float().cuda())
    gots = (v.grad, sr.grad, dr.grad) if tri else (v.grad,)
    for name, got, ref in zip(("volume", "source", "directions"), gots, refs):
        assert got is not None and got.abs().sum() > 0, name
        assert maxnorm_rel(got.cpu().numpy(), ref.cpu().numpy()) <= 1e-5, name


@pytest.mark.gpu
def test_graph_capture_forward_and_backward():
    """one stream, no parallel branches: a loss over apply_artifacts and its backward captured once (the pattern of
    the other capture tests: warm-up on a side stream, `.backward()` of a scalar built inside the capture), replayed,
    equal to eager"""
    import diffus_amd
    rng = np.random.default_rng(8)
    f = torch.from_numpy(rng.normal(0.3, 1.0, size=(4, 64, 128)).astype(np.float32)).cuda().requires_grad_(True)
    w = torch.from_numpy(rng.normal(size=(4, 64, 128))).cuda()
    out = torch.zeros((4, 64, 128), dtype=torch.float64, device="cuda")

    def step():
        y = diffus_amd.apply_artifacts(f, seed=21)
        (y * w).sum().backward()
        out.copy_(y.detach())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            f.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_y, want_g = out.clone(), f.grad.clone()
    g = torch.cuda.CUDAGraph()
    f.grad = None
    out.zero_()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_y) and torch.equal(f.grad, want_g)
