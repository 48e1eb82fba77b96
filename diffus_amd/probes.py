"""Linear and convex array probes: one beam ORIGIN per ray.

A sector fan (cone.py, FanPose) has one apex per pose.  Linear arrays (vascular, musculoskeletal, small parts) fire parallel
beams from elements spread along a line; convex arrays (abdominal) fire radial beams from elements on an arc.  Both hand
`render_poses` / `trace_rays` / `CapturedStep` per-ray sources (P,R,3), which the kernels take as DIFFUS_SRC_PER_RAY
(include/diffus_hip.h): ray r of pose p walks src[p, r] + k * dirs[p, r] with the reference's roundings
(src/renderer.py:119-124).

Everything here is a handful of differentiable torch ops per step, in the dtype of the inputs (float64 stays float64).
"""
from __future__ import annotations

import torch

from .cone import rotation_from_rotvec


def _vec(x, dtype=None, device=None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x if dtype is None else x.to(dtype)
    return torch.as_tensor(x, dtype=dtype or torch.get_default_dtype(), device=device)


def _unit(v: torch.Tensor) -> torch.Tensor:
    return v / torch.linalg.vector_norm(v, dim=-1, keepdim=True)


def _frame(center, axial, lateral):
    """(center, unit axial, unit lateral made orthogonal to axial), in one dtype (torch promotion of the three)."""
    ts = [x for x in (center, axial, lateral) if isinstance(x, torch.Tensor)]
    dt = torch.get_default_dtype()
    for t in ts:
        dt = torch.promote_types(dt, t.dtype) if t.is_floating_point() else dt
    dev = ts[0].device if ts else None
    c, a, l = (_vec(x, dt, dev) for x in (center, axial, lateral))
    a = _unit(a)
    l = _unit(l - (l * a).sum(-1, keepdim=True) * a)
    return c, a, l


def _spread(n: int, like: torch.Tensor) -> torch.Tensor:
    """n values evenly spaced over [-1/2, 1/2] (0 for one element)."""
    if n < 1:
        raise ValueError("n_elements must be at least 1")
    if n == 1:
        return torch.zeros(1, dtype=like.dtype, device=like.device)
    return torch.arange(n, dtype=like.dtype, device=like.device) / (n - 1) - 0.5


def linear_array(center, axial, lateral, n_elements: int, width):
    """A linear array: `n_elements` elements evenly spaced along `lateral` (made orthogonal to `axial`), the first and the
    last `width` apart and centred on `center`; every beam points along `axial`.
    -> sources (R,3), directions (R,3), R = n_elements."""
    c, a, l = _frame(center, axial, lateral)
    t = _spread(int(n_elements), c) * width
    sources = c + t[:, None] * l
    directions = a.expand(int(n_elements), 3)
    return sources, directions


def convex_array(center_of_curvature, axial, lateral, radius, opening_angle, n_elements: int):
    """A convex (curvilinear) array: `n_elements` elements on the arc of radius `radius` about `center_of_curvature`, in
    the plane of `axial` and `lateral`, at angles evenly spaced over `opening_angle` (radians) about `axial`; every beam
    points radially outward from the centre of curvature.
    -> sources (R,3), directions (R,3), R = n_elements."""
    c, a, l = _frame(center_of_curvature, axial, lateral)
    th = _spread(int(n_elements), c) * opening_angle
    directions = torch.cos(th)[:, None] * a + torch.sin(th)[:, None] * l
    sources = c + radius * directions
    return sources, directions


class ArrayPose(torch.nn.Module):
    """Differentiable pose of an array probe, batched over P poses like FanPose.

    The element layout is fixed in the probe frame: `offsets` (R,3) from the probe origin and `directions` (R,3), e.g.
    `src, dirs = linear_array(c, ...)` and `ArrayPose(c, src - c, dirs)`.  The parameters are the probe origin (P,3) and,
    unless `rotvec` is None, a rotation vector (P,3) (axis x angle, radians, rotation_from_rotvec) turning the probe about
    its origin:  sources[p, r] = origin[p] + R_p offsets[r],  directions[p, r] = R_p directions[r].
    forward() -> sources (P,R,3), directions (P,R,3) -- per-ray sources for render_poses.  A single pose (origin (3,))
    gives P = 1.
    """

    def __init__(self, origin, offsets, directions, rotvec=None):
        super().__init__()
        o = _vec(origin).detach().clone()
        self.origin = torch.nn.Parameter(o if o.dim() == 2 else o.reshape(1, 3))
        self.register_buffer("offsets", _vec(offsets, self.origin.dtype).detach().clone())
        self.register_buffer("element_directions", _vec(directions, self.origin.dtype).detach().clone())
        if self.offsets.dim() != 2 or self.offsets.shape != self.element_directions.shape or self.offsets.shape[1] != 3:
            raise ValueError("offsets and directions must both be (R,3)")
        if rotvec is None:
            self.rotvec = None
        else:
            rv = _vec(rotvec, self.origin.dtype).detach().clone().reshape(-1, 3)
            if rv.shape[0] != self.origin.shape[0]:
                rv = rv.expand(self.origin.shape[0], 3).clone()
            self.rotvec = torch.nn.Parameter(rv)
        # an array in one slice, moved in that slice only: dim-2 directions exact zeros and one dim-2 coordinate per pose
        self._in_plane = (self.rotvec is None and bool((self.element_directions[:, 2] == 0).all())
                          and bool((self.offsets[:, 2] == self.offsets[0, 2]).all()))

    def forward(self):
        P = self.origin.shape[0]
        if self.rotvec is None:
            sources = self.origin[:, None, :] + self.offsets
            directions = self.element_directions.expand(P, -1, -1)
        else:
            rot = torch.stack([rotation_from_rotvec(self.rotvec[p]) for p in range(P)])       # (P,3,3)
            sources = self.origin[:, None, :] + torch.einsum("pij,rj->pri", rot, self.offsets)
            directions = torch.einsum("pij,rj->pri", rot, self.element_directions)
        if self._in_plane:
            # exact zeros / one level by construction: tell the renderer (renderer._fans_planar, _sources_level), which does
            # not read back tensors that require grad
            sources._diffus_planar = True
            directions._diffus_planar = True
        return sources, directions
