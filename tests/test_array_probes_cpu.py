"""Linear and convex array probes without a GPU: the DIFFUS_SRC_PER_RAY flag bit of the C ABI is validated before anything
touches HIP, and the geometry helpers / ArrayPose (diffus_amd/probes.py) are plain torch."""
import ctypes as C
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from diffus_amd import build, _lib
    build.build()
    return _lib.load()


def test_src_per_ray_flag_is_declared_and_the_abi_stays_8(lib):
    from diffus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "diffus_hip.h")).read()
    assert "#define DIFFUS_SRC_PER_RAY 0x10" in txt
    assert _lib.SRC_PER_RAY == 0x10
    assert lib.diffus_abi_version() == _lib.ABI_VERSION == 8
    for n in _lib.EXPORTS:
        assert getattr(lib, n) is not None


def test_src_per_ray_flag_validation_without_a_gpu(lib):
    f = (C.c_float * 64)()
    p = C.cast(f, C.c_void_p)
    PR = 0x10

    def fwd(sdt, frame=p):
        return lib.diffus_render_fwd(p, 2, 2, 2, 0, p, sdt, p, 0, 1, 2, 4, 0, 0.1, 0, frame, None, None, 0, None)

    assert fwd(3) == -1                      # invalid low bits, no flag
    assert fwd(PR | 2) == -1                 # per-ray with a bad dtype (I64 is no pose dtype)
    assert fwd(PR | 3) == -1
    assert fwd(0x40) == -1                   # an unknown bit
    assert fwd(PR | 0x40) == -1
    assert fwd(PR, frame=None) == -1         # null frame
    assert fwd(PR | 1, frame=None) == -1
    for sdt in (PR | 2, 0x40):
        assert lib.diffus_trace_rays(p, 2, 2, 2, 0, p, sdt, p, 0, 1, 2, 4, 0, p, None, None, None) == -1
        assert lib.diffus_trace_rays_bwd(p, 2, 2, 2, 0, p, sdt, p, 0, 1, 2, 4, 1, p, None, None, p, None, None, 0, None) == -1
        assert lib.diffus_render_bwd(p, 2, 2, 2, 0, p, sdt, p, 0, 1, 2, 4, 0, 0.1, 0, p, p, None, None, None, 3, p, 1 << 20,
                                     None) == -1
        assert lib.diffus_render_bwd_mse(p, 2, 2, 2, 0, p, sdt, p, 0, 1, 2, 4, 0, 0.1, 0, p, None, 1.0, p, p, None, None, None,
                                         3, p, 1 << 20, None) == -1
        assert lib.diffus_render_step_mse(p, 2, 2, 2, 0, p, sdt, p, 0, 1, 2, 4, 0, 0.1, 0, None, 1.0, p, p, p, None, None,
                                          None, 3, p, 1 << 20, None) == -1
    # valid flag, nothing to compute: accepted without a launch
    assert lib.diffus_trace_rays(p, 2, 2, 2, 0, p, PR, p, 0, 1, 2, 4, 0, None, None, None, None) == 0
    assert lib.diffus_trace_rays(p, 2, 2, 2, 0, p, PR | 1, p, 1, 1, 2, 4, 0, None, None, None, None) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_linear_array_spacing_and_directions(dtype):
    from diffus_amd import linear_array
    c = torch.tensor([30.0, 20.0, 11.5], dtype=dtype)
    src, dirs = linear_array(c, torch.tensor([2.0, 0.0, 0.0], dtype=dtype), torch.tensor([0.3, 1.0, 0.0], dtype=dtype), 9, 16.0)
    assert src.shape == (9, 3) and dirs.shape == (9, 3) and src.dtype == dtype and dirs.dtype == dtype
    steps = src[1:] - src[:-1]
    torch.testing.assert_close(steps.norm(dim=1), torch.full((8,), 2.0, dtype=dtype))      # 16 / (9 - 1)
    torch.testing.assert_close(steps, steps[:1].expand(8, 3))                               # evenly spaced on one line
    torch.testing.assert_close(src.mean(0), c)
    torch.testing.assert_close(dirs, torch.tensor([[1.0, 0.0, 0.0]], dtype=dtype).expand(9, 3))
    assert torch.allclose((steps[0] * dirs[0]).sum(), torch.zeros((), dtype=dtype), atol=1e-6)  # lateral made orthogonal


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_convex_array_elements_on_the_arc_with_radial_beams(dtype):
    from diffus_amd import convex_array
    c = torch.tensor([5.0, 32.0, 20.0], dtype=dtype)
    radius, opening, n = 12.0, 1.1, 7
    src, dirs = convex_array(c, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], radius, opening, n)
    assert src.shape == (n, 3) and src.dtype == dtype
    tol = dict(rtol=1e-6, atol=1e-6) if dtype == torch.float32 else dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dirs.norm(dim=1), torch.ones(n, dtype=dtype), **tol)
    torch.testing.assert_close(src - c, radius * dirs, **tol)                            # radial: origin on the beam's line
    ang = torch.atan2(dirs[:, 1], dirs[:, 0])
    torch.testing.assert_close(ang[1:] - ang[:-1], torch.full((n - 1,), opening / (n - 1), dtype=dtype), **tol)
    torch.testing.assert_close(ang[0], torch.tensor(-opening / 2, dtype=dtype), **tol)


def test_array_pose_at_identity_equals_the_helpers():
    from diffus_amd import ArrayPose, convex_array, linear_array
    c = torch.tensor([30.0, 20.0, 11.0], dtype=torch.float64)
    for src, dirs in (linear_array(c, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], 8, 10.0),
                      convex_array(c, [1.0, 0.2, 0.0], [0.0, 1.0, 0.0], 9.0, 0.8, 6)):
        for rv in (None, torch.zeros(2, 3, dtype=torch.float64)):
            pose = ArrayPose(c.expand(2, 3), src - c, dirs, rotvec=rv)
            s, d = pose()
            assert s.shape == (2, src.shape[0], 3) and d.shape == s.shape
            torch.testing.assert_close(s, src.expand(2, -1, -1), rtol=0, atol=1e-13)
            torch.testing.assert_close(d, dirs.expand(2, -1, -1), rtol=0, atol=1e-15)
            # in the slice and only translated: marked for the renderer's planar hint
            assert getattr(d, "_diffus_planar", False) == (rv is None)


def test_array_pose_rotation_turns_the_layout_about_the_origin():
    from diffus_amd import ArrayPose, linear_array
    c = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64)
    src, dirs = linear_array(c, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], 3, 2.0)
    pose = ArrayPose(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), src, dirs,
                     rotvec=torch.tensor([0.0, 0.0, math.pi / 2], dtype=torch.float64))
    s, d = pose()
    torch.testing.assert_close(d[0], torch.tensor([[0.0, 1.0, 0.0]] * 3, dtype=torch.float64), rtol=0, atol=1e-12)
    torch.testing.assert_close(s[0], torch.tensor([[2.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 2.0, 3.0]], dtype=torch.float64),
                               rtol=0, atol=1e-12)


def test_array_pose_float64_gradients_match_finite_differences():
    from diffus_amd import ArrayPose, convex_array
    c = torch.tensor([10.0, 12.0, 9.0], dtype=torch.float64)
    src, dirs = convex_array(c, [1.0, 0.0, 0.1], [0.0, 1.0, 0.0], 7.0, 0.9, 5)
    pose = ArrayPose(torch.tensor([[10.0, 12.0, 9.0], [11.0, 13.0, 8.0]], dtype=torch.float64), src - c, dirs,
                     rotvec=torch.tensor([[0.05, -0.02, 0.3], [0.0, 0.0, 0.0]], dtype=torch.float64))
    w1 = torch.randn(2, 5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    w2 = torch.randn(2, 5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))

    def loss(origin, rotvec):
        with torch.no_grad():
            pose.origin.copy_(origin)
            pose.rotvec.copy_(rotvec)
        s, d = pose()
        return (s * w1).sum() + (d * w2).sum() * 10.0

    o0, r0 = pose.origin.detach().clone(), pose.rotvec.detach().clone()
    pose.zero_grad()
    loss(o0, r0).backward()
    go, gr = pose.origin.grad.clone(), pose.rotvec.grad.clone()
    h = 1e-6
    for (name, base, g) in (("origin", o0, go), ("rotvec", r0, gr)):
        fd = torch.zeros_like(base)
        for i in range(base.numel()):
            e = torch.zeros_like(base).view(-1)
            e[i] = h
            e = e.view_as(base)
            with torch.no_grad():
                plus = loss(o0 + e, r0) if name == "origin" else loss(o0, r0 + e)
                minus = loss(o0 - e, r0) if name == "origin" else loss(o0, r0 - e)
            fd.view(-1)[i] = (plus - minus) / (2 * h)
        torch.testing.assert_close(g, fd, rtol=1e-6, atol=1e-7)
