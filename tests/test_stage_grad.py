"""Gradients through the stage-level functions (custom_nearest_sampler, trace_rays / trace_ray / simulate_rays,
compute_gaussian_pulse): diffus_sample_points_bwd, diffus_trace_rays_bwd, diffus_rows_conv1d_bwd.

"Correct" is float64 torch autograd over oracle.autograd_ref's restatements (sample_nearest, sample_trilinear,
reflection, echo_scan) at the float32 points the reference samples, the reference's own autograd for golden G7, and
render_poses' backward for the composed path at start = 0."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, maxnorm_rel
from diffus_amd.phantom import phantom, pose_ring
from oracle import autograd_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da():
    import diffus_amd
    return diffus_amd


def rel(a, b):
    return maxnorm_rel(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def ref_points(src, dirs, S):
    """Where the reference samples (source + steps * dirs with torch's promotion: float32 steps and directions, the
    source's dtype for the add; cast to float32 by the sampler), carried in float64 with the exact derivatives."""
    steps = torch.arange(S, dtype=torch.float32).view(1, S, 1)
    with torch.no_grad():
        p = (src.detach().cpu().view(1, 1, 3) + steps * dirs.detach().cpu().float().unsqueeze(1)).float()
    exact = ar.ray_points(src.cpu().double(), dirs.cpu().double(), S)
    return p.double() + (exact - exact.detach())


def ref_trace(vol64, src, dirs, S, sampler):
    """float64 (imp (R,S), refl (R,S-1)) of one pose, differentiable in vol64 / src / dirs (leaves on the CPU)."""
    pts = ref_points(src, dirs, S)
    imp = ar.sample_nearest(vol64, pts)[0] if sampler == "nearest" else ar.sample_trilinear(vol64, pts)
    return imp, ar.reflection(imp)


# ---------------------------------------------------------------- 1. golden G7 through the composed path
def _g7_frame(e, alpha):
    return e * torch.exp(-alpha * torch.arange(e.shape[1]).float())[None, :]


@pytest.mark.parametrize("how", ["sampler", "simulate_rays"])
def test_g7_composed_path_matches_the_reference_autograd(da, how):
    g = load_golden("g7_volume_grad")
    n, S, alpha = int(g["n"]), int(g["S"]), float(g["alpha"])
    v = torch.from_numpy(phantom(n)).clone().requires_grad_(True)          # CPU tensors end to end, as make_golden.py
    src_t, dir_t = torch.from_numpy(g["source"]), torch.from_numpy(g["directions"])
    if how == "sampler":
        steps = torch.arange(0, S, dtype=torch.float32).view(1, -1, 1)
        pts = src_t + steps * dir_t.unsqueeze(1)
        x, y, z, imp = da.custom_nearest_sampler(v, pts, visualize=False)
        r = da.UltrasoundRenderer.compute_reflection_coeff(imp[:, :-1], imp[:, 1:])
    else:
        x, y, z, r = da.UltrasoundRenderer(S, alpha).simulate_rays(v, src_t, dir_t)
    assert r.grad_fn is not None and x.dtype == torch.int64 and not x.requires_grad
    e, _ = da.compute_echo_traces(r)
    frame = _g7_frame(e, alpha)
    assert maxnorm_rel(frame.detach().numpy(), g["frame"]) <= 1e-4
    (frame ** 2).sum().backward()
    ref = np.zeros(n ** 3, dtype=np.float64)
    ref[g["grad_index"]] = g["grad_value"]
    assert v.grad is not None and v.grad.device.type == "cpu"
    assert maxnorm_rel(v.grad.flatten().numpy(), ref) <= 1e-3


# ---------------------------------------------------------------- 2. nearest sampler against torch indexing
@pytest.mark.parametrize("zdt", [torch.float32, torch.float64])
def test_nearest_sampler_grad_is_torch_indexing(da, zdt):
    g16 = load_golden("g16_api_functions")
    vol, pts = torch.from_numpy(g16["vol"]), torch.from_numpy(g16["pts"])
    w = torch.randn(pts.shape[:2], generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    Z = vol.to(zdt).cuda().requires_grad_(True)
    P = pts.cuda().requires_grad_(True)
    x, y, z, v = da.custom_nearest_sampler(Z, P, visualize=False)
    assert v.dtype == zdt and v.grad_fn is not None
    assert np.array_equal(v.detach().float().cpu().numpy(), g16["sv"]) and np.array_equal(x.cpu().numpy(), g16["sx"])
    (v.double().cpu() * w).sum().backward()
    Z64 = vol.double().requires_grad_(True)
    idx = [torch.from_numpy(g16[k]) for k in ("sx", "sy", "sz")]
    (Z64[idx[0], idx[1], idx[2]] * w).sum().backward()
    assert Z.grad.dtype == zdt
    assert rel(Z.grad, Z64.grad) <= 1e-6
    assert P.grad is None                       # .round().long() cuts the points' graph in the reference


def test_nearest_sampler_points_alone_record_nothing(da):
    g16 = load_golden("g16_api_functions")
    P = torch.from_numpy(g16["pts"]).cuda().requires_grad_(True)
    *_, v = da.custom_nearest_sampler(torch.from_numpy(g16["vol"]).cuda(), P, visualize=False)
    assert v.grad_fn is None


# ---------------------------------------------------------------- 3. trilinear sampler
def _tri_case(da, vol, pts, seed):
    w = torch.randn(pts.shape[:2], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    Z = vol.cuda().requires_grad_(True)
    P = pts.cuda().requires_grad_(True)
    *_, v = da.custom_nearest_sampler(Z, P, visualize=False, sampler="trilinear")
    (v.double().cpu() * w).sum().backward()
    Z64 = vol.double().requires_grad_(True)
    P64 = pts.double().requires_grad_(True)
    (ar.sample_trilinear(Z64, P64) * w).sum().backward()
    return Z, P, Z64, P64


def test_trilinear_sampler_grads_against_float64_autograd(da):
    g = torch.Generator().manual_seed(3)
    vol = torch.rand(9, 11, 13, generator=g) * 1e6 + 1e6
    pts = torch.rand(6, 40, 3, generator=g) * torch.tensor([8.0, 10.0, 12.0])
    pts = torch.where((pts - pts.round()).abs() < 1e-3, pts + 0.01, pts)          # away from ties
    Z, P, Z64, P64 = _tri_case(da, vol, pts, 4)
    assert rel(Z.grad, Z64.grad) <= 1e-5
    assert rel(P.grad, P64.grad) <= 1e-4


def test_trilinear_sampler_border_rule(da):
    """Points on and beyond every face.  Beyond a face, and on the upper one, no gradient along that axis, as torch's
    clamp gives.  ON the lower face (p == 0 exactly) the kernels' border rule (tri_sample<..., true>, the rule of
    render_poses: no gradient where p <= 0 or p >= dim - 1) passes nothing, where torch's clamp passes the one-sided
    derivative: that component is masked out of the comparison."""
    g = torch.Generator().manual_seed(5)
    vol = torch.rand(5, 6, 7, generator=g) + 1.0
    hi = torch.tensor([4.0, 5.0, 6.0])
    vals = [lambda h: -1.5, lambda h: 0.0, lambda h: h, lambda h: h + 0.7, lambda h: 1.3, lambda h: h - 0.4]
    rows = []
    for a in range(3):
        for f in vals:
            for b in vals[4:]:
                p = torch.tensor([b(hi[c]) for c in range(3)])
                p[a] = f(hi[a])
                rows.append(p)
    pts = torch.stack(rows).view(1, -1, 3).float()
    Z, P, Z64, P64 = _tri_case(da, vol, pts, 6)
    assert rel(Z.grad, Z64.grad) <= 1e-5
    want = torch.where(pts.double() == 0, torch.zeros_like(P64.grad), P64.grad)
    assert rel(P.grad, want) <= 1e-4
    beyond = (pts < 0) | (pts >= hi) | (pts == 0)
    assert (P.grad.cpu()[beyond] == 0).all()


# ---------------------------------------------------------------- 4. trace_rays / trace_ray / simulate_rays
def _ref_trace_grads(vol, src, dirs, S, sampler, wi, wr, shared):
    """float64 autograd of sum(wi * imp) + sum(wr * refl) over every pose."""
    v64 = torch.from_numpy(vol).double().requires_grad_(True)
    s64 = src.detach().cpu().clone().requires_grad_(True)
    d64 = dirs.detach().cpu().clone().requires_grad_(True)
    loss = 0
    for p in range(s64.shape[0]):
        imp, refl = ref_trace(v64, s64[p], d64 if shared else d64[p], S, sampler)
        loss = loss + (imp * wi[p]).sum() + (refl * wr[p]).sum()
    loss.backward()
    return v64.grad, s64.grad, d64.grad


@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
@pytest.mark.parametrize("P,shared,sdt", [(1, False, torch.float32), (5, False, torch.float32), (5, True, torch.float32),
                                          (3, False, torch.float64)])
def test_trace_rays_grads_against_float64_autograd(da, sampler, P, shared, sdt):
    n, R, S = 32, 12, 40
    vol = phantom(n)
    src, dirs = pose_ring(n, P, R)
    g = torch.Generator().manual_seed(P + 7 * shared)
    wi = torch.randn(P, R, S, generator=g, dtype=torch.float64)
    wr = torch.randn(P, R, S - 1, generator=g, dtype=torch.float64) * 1e6     # d refl / d Z ~ 1 / Z
    V = torch.from_numpy(vol).cuda().requires_grad_(True)
    s = torch.from_numpy(src).to(sdt).cuda().requires_grad_(True)
    d = torch.from_numpy(dirs[0] if shared else dirs).cuda().requires_grad_(True)
    grads = []
    for _ in range(2):
        V.grad = s.grad = d.grad = None
        out = da.trace_rays(V, s, d, S, sampler)
        assert out["imp"].grad_fn is not None and out["idx"].grad_fn is None
        loss = (out["imp"].double().cpu() * wi).sum() + (out["refl"].double().cpu() * wr).sum()
        loss.backward()
        grads.append((V.grad.clone(), s.grad.clone(), d.grad.clone()))
    gv, gs, gd = grads[0]
    assert gs.dtype == sdt and gs.shape == s.shape and gd.shape == d.shape and gv.dtype == torch.float32
    assert torch.equal(gs, grads[1][1]) and torch.equal(gd, grads[1][2])      # fixed-order pose sums
    rv, rs, rd = _ref_trace_grads(vol, s, d, S, sampler, wi, wr, shared)
    assert rel(gv, rv) <= 1e-4
    if sampler == "trilinear":
        assert rel(gs, rs) <= 1e-4 and rel(gd, rd) <= 1e-4
    else:                                   # nearest: zeros, as render_poses gives
        assert not gs.any() and not gd.any()


@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
def test_trace_ray_and_simulate_rays_grads(da, sampler):
    n, R, S = 32, 10, 30
    vol = phantom(n)
    src, dirs = pose_ring(n, 2, R)
    s1, d1 = torch.from_numpy(src[1]), torch.from_numpy(dirs[1])
    rr = da.UltrasoundRenderer(num_samples=S, attenuation_coeff=1e-3)
    g = torch.Generator().manual_seed(11)
    for case in ("trace_ray", "simulate_rays", "mri", "one_ray"):
        V = torch.from_numpy(vol).cuda().requires_grad_(True)
        s = s1.clone().requires_grad_(True)
        d = (d1[:1] if case == "one_ray" else d1).clone().requires_grad_(True)
        if case == "trace_ray":
            out = da.UltrasoundRenderer.trace_ray(V, s, d, S, 0, sampler=sampler)[3]
        elif case == "mri":
            out = rr.simulate_rays(V, s, d, MRI=True, sampler=sampler)
        else:
            out = rr.simulate_rays(V, s, d, sampler=sampler)[3]
        if case == "one_ray":
            assert out.dim() == 1
        w = torch.randn(out.shape, generator=g, dtype=torch.float64) * (1.0 if case in ("trace_ray", "mri") else 1e6)
        (out.double().cpu() * w).sum().backward()
        v64 = torch.from_numpy(vol).double().requires_grad_(True)
        s64, d64 = s1.clone().double().requires_grad_(True), d.detach().clone().requires_grad_(True)
        imp, refl = ref_trace(v64, s64, d64, S, sampler)
        ref = {"trace_ray": imp, "mri": imp[:, :-1], "simulate_rays": refl, "one_ray": refl.squeeze(0)}[case]
        (ref * w).sum().backward()
        assert rel(V.grad, v64.grad) <= 1e-4, case
        if sampler == "trilinear":
            assert rel(s.grad, s64.grad) <= 1e-4 and rel(d.grad, d64.grad) <= 1e-4, case
        assert s.grad.dtype == torch.float32 and s.grad.device.type == "cpu"


def test_reflection_grad_where_impedances_sum_to_zero(da):
    """Z1 + Z2 = 0 (air-like pairs of opposite sign, and 0/0): the volume gradient is what torch's float32 autograd gives
    through compute_reflection_coeff -- the same inf / NaN, bit for bit elsewhere."""
    vals = torch.tensor([1.0, -1.0, 2.0, 0.0, 0.0, 3.0, -3.0, 5.0, 0.5, -0.5])
    S = vals.numel()
    w = torch.randn(S - 1, generator=torch.Generator().manual_seed(13))
    imp = vals.clone().requires_grad_(True)
    r = da.UltrasoundRenderer.compute_reflection_coeff(imp[:-1], imp[1:])
    r.backward(w)
    V = vals.view(1, 1, S).cuda().requires_grad_(True)
    src, d = torch.zeros(3), torch.tensor([[0.0, 0.0, 1.0]])          # one ray along dim 2, one voxel per step
    out = da.trace_rays(V, src, d, S, "nearest", want=("refl",), layout="canonical")["refl"]
    torch.testing.assert_close(out.detach().cpu().view(-1), r.detach(), rtol=0, atol=0, equal_nan=True)
    out.backward(w.view(1, 1, -1).cuda())
    got = V.grad.view(-1).cpu()
    assert not torch.isfinite(imp.grad).all()                         # the case is really exercised
    torch.testing.assert_close(got, imp.grad, rtol=0, atol=0, equal_nan=True)


def test_integer_volume_with_points_that_require_grad(da):
    """An integer Z gives float32 values whether or not the points require grad (trilinear: they get a gradient)."""
    g = torch.Generator().manual_seed(9)
    Z = torch.randint(0, 100, (6, 7, 8), generator=g)
    pts = (torch.rand(2, 9, 3, generator=g) * torch.tensor([5.0, 6.0, 7.0])).requires_grad_(True)
    *_, v = da.custom_nearest_sampler(Z, pts, visualize=False, sampler="trilinear")
    *_, v0 = da.custom_nearest_sampler(Z, pts.detach(), visualize=False, sampler="trilinear")
    assert v.dtype == torch.float32 and torch.equal(v.detach(), v0) and v.grad_fn is not None
    v.sum().backward()
    P64 = pts.detach().double().requires_grad_(True)
    ar.sample_trilinear(Z.double(), P64).sum().backward()
    assert rel(pts.grad, P64.grad) <= 1e-4


# ---------------------------------------------------------------- 5. the composed path equals render_poses' backward
@pytest.mark.parametrize("sampler", ["nearest", "trilinear"])
def test_composed_path_matches_render_poses(da, sampler):
    n, P, R, S, alpha = 64, 3, 16, 64, 1e-3
    src, dirs = pose_ring(n, P, R)
    base = torch.from_numpy(phantom(n)).cuda()
    res = []
    for path in ("composed", "render_poses"):
        V = base.clone().requires_grad_(True)
        s = torch.from_numpy(src).cuda().requires_grad_(True)
        d = torch.from_numpy(dirs).cuda().requires_grad_(True)
        if path == "composed":
            r = da.trace_rays(V, s, d, S, sampler, want=("refl",))["refl"]
            e, _ = da.compute_echo_traces(r.reshape(P * R, S - 1))
            frame = (e * torch.exp(-alpha * torch.arange(S, device="cuda").float())[None, :]).reshape(P, R, S)
        else:
            frame = da.render_poses(V, s, d, S, alpha, start=0, sampler=sampler)
        (frame ** 2).sum().backward()
        res.append((frame.detach(), V.grad, s.grad, d.grad))
    assert rel(res[0][0], res[1][0]) <= 1e-4
    for a, b in zip(res[0][1:], res[1][1:]):
        assert rel(a, b) <= 1e-3


# ---------------------------------------------------------------- 6. pulse
@pytest.mark.parametrize("j", [0, 1, 2])
def test_gaussian_pulse_grads(da, j):
    g13 = load_golden("g13_gaussian_pulse")
    length, sigma = (int(x) for x in g13[f"p{j}"])
    r0 = torch.from_numpy(g13["r"])
    taps = torch.from_numpy(g13[f"pulse{j}"]).float().view(1, 1, -1)
    w = torch.randn(g13[f"out{j}"].shape, generator=torch.Generator().manual_seed(j), dtype=torch.float64)
    got = []
    for _ in range(2):
        r = r0.clone().cuda().requires_grad_(True)
        pulse = taps.clone().cuda().requires_grad_(True)
        out = da.compute_gaussian_pulse(r, length=length, sigma=sigma, pulse=pulse)
        assert maxnorm_rel(out.detach().cpu().numpy(), g13[f"out{j}"]) <= 1e-5
        (out.double().cpu() * w).sum().backward()
        got.append((r.grad, pulse.grad))
    assert torch.equal(got[0][1], got[1][1])                          # fixed-order pulse gradient
    r64 = r0.double().requires_grad_(True)
    p64 = taps.double().requires_grad_(True)
    ref = F.conv1d(ar.echo_scan(r64).unsqueeze(1), p64, padding=length // 2).squeeze(1)
    (ref * w).sum().backward()
    assert got[0][1].shape == taps.shape and got[0][1].dtype == torch.float32
    assert rel(got[0][0], r64.grad) <= 1e-5
    assert rel(got[0][1], p64.grad) <= 1e-5


def test_gaussian_pulse_default_pulse_grad_to_refLR(da):
    g13 = load_golden("g13_gaussian_pulse")
    r = torch.from_numpy(g13["r"]).requires_grad_(True)                  # CPU, default pulse
    out = da.compute_gaussian_pulse(r, length=7, sigma=2)
    assert out.grad_fn is not None
    out.sum().backward()
    r64 = torch.from_numpy(g13["r"]).double().requires_grad_(True)
    k = torch.from_numpy(da.gaussian_pulse(7, 2)).view(1, 1, -1)
    F.conv1d(ar.echo_scan(r64).unsqueeze(1), k, padding=3).sum().backward()
    assert rel(r.grad, r64.grad) <= 1e-5


# ---------------------------------------------------------------- 7. calls without grad take today's path
def test_no_grad_outputs_unchanged(da):
    n, S = 32, 30
    src, dirs = pose_ring(n, 2, 8)
    vol = torch.from_numpy(phantom(n)).cuda()
    s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dirs).cuda()
    g16 = load_golden("g16_api_functions")
    Z, pts = torch.from_numpy(g16["vol"]).cuda(), torch.from_numpy(g16["pts"]).cuda()
    r = torch.from_numpy(load_golden("g13_gaussian_pulse")["r"]).cuda()
    pulse = torch.from_numpy(da.gaussian_pulse(10, 1)).float().view(1, 1, -1).cuda()

    def run(vv, ss, dd, zz, pp, rr, kk):
        outs = []
        for sm in ("nearest", "trilinear"):
            o = da.trace_rays(vv, ss, dd, S, sm)
            outs += [o["imp"], o["refl"], o["idx"]]
            outs += list(da.custom_nearest_sampler(zz, pp, visualize=False, sampler=sm))
        outs.append(da.compute_gaussian_pulse(rr, pulse=kk))
        return outs

    plain = run(vol, s, d, Z, pts, r, pulse)
    with torch.no_grad():
        ng = run(vol, s, d, Z, pts, r, pulse)
    graded = run(vol.clone().requires_grad_(True), s.clone().requires_grad_(True), d.clone().requires_grad_(True),
                 Z.clone().requires_grad_(True), pts.clone().requires_grad_(True), r.clone().requires_grad_(True),
                 pulse.clone().requires_grad_(True))
    for a, b, c in zip(plain, ng, graded):
        assert a.grad_fn is None
        assert torch.equal(a, b) and torch.equal(a, c.detach())
    assert graded[0].grad_fn is not None and graded[-1].grad_fn is not None


def test_in_place_edit_between_forward_and_backward_raises(da):
    n, S = 32, 20
    src, dirs = pose_ring(n, 1, 4)
    V = torch.from_numpy(phantom(n)).cuda().requires_grad_(True)
    d = torch.from_numpy(dirs).cuda()
    out = da.trace_rays(V, torch.from_numpy(src).cuda(), d, S, "trilinear", layout="canonical")
    with torch.no_grad():
        V.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        out["imp"].sum().backward()


# ---------------------------------------------------------------- 8. graph capture
def test_composed_path_graph_capture(da):
    n, P, R, S, alpha = 64, 2, 16, 48, 1e-3
    src, dirs = pose_ring(n, P, R)
    V = torch.from_numpy(phantom(n)).cuda().requires_grad_(True)
    s = torch.from_numpy(src).cuda()
    d = torch.from_numpy(dirs).cuda().requires_grad_(True)
    att = torch.exp(-alpha * torch.arange(S, device="cuda").float())[None, :]

    def step():
        r = da.trace_rays(V, s, d, S, "trilinear", want=("refl",))["refl"]
        e, _ = da.compute_echo_traces(r.reshape(P * R, S - 1))
        ((e * att) ** 2).sum().backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            V.grad = d.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_v, want_d = V.grad.clone(), d.grad.clone()
    g = torch.cuda.CUDAGraph()
    V.grad = d.grad = None
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(d.grad, want_d)
    assert rel(V.grad, want_v) <= 1e-6
