"""B-mode artifact chain on the GPU: mirror of what plot_beam_frame(artifacts=True) does in the
reference (src/renderer.py:264-273) -- speckle arcs, depth-dependent lateral blur, unsharp mask --
over diffus_artifacts.  Returns float64 like the reference.  The reference draws its speckle from
the unseeded global NumPy RNG; here `seed` makes a frame reproducible, and `noise=(radial, local)`
injects explicit factors (used by the parity tests with the very draws the reference made).

Unlike the reference (NumPy/SciPy), the chain is differentiable in the frames: with grad enabled and
`frames.requires_grad`, the result carries an autograd node whose backward is diffus_artifacts_bwd.
`artifact_noise` hands out the factors a seeded call multiplies by."""
from __future__ import annotations

import itertools

import torch

from . import _lib
from .renderer import _Scope, _as, _device_for, _ptr, _stream, _workspace

_auto_seed = itertools.count(0x5EED)


def _launch(frames, std_radial, std_local, max_sigma, alpha, seed, noise):
    """diffus_artifacts -> (out (P,R,N) float64, the launch's inputs for a backward)."""
    lib = _lib.load()
    dev = _device_for(frames)
    f = _as(frames, dev, torch.float32)
    if f.dim() == 2:
        f = f.unsqueeze(0)
    P, R, N = f.shape
    if N > 1 and not (max_sigma > 0):
        raise ZeroDivisionError("float division by zero")      # what SciPy raises in the reference for sigma = 0
    rad = loc = None
    if noise is not None:
        rad = torch.as_tensor(noise[0], dtype=torch.float64, device=dev).reshape(P, N).contiguous()
        loc = torch.as_tensor(noise[1], dtype=torch.float64, device=dev).reshape(P, R, N).contiguous()
    if seed is None:
        seed = next(_auto_seed)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with _Scope(dev):
        out = torch.empty((P, R, N), dtype=torch.float64, device=dev)
        ws = _workspace(dev, lib.diffus_artifacts_workspace_bytes(P, R, N))
        rc = lib.diffus_artifacts(_ptr(f), P, R, N, float(std_radial), float(std_local), float(max_sigma), float(alpha),
                                  _ptr(rad), _ptr(loc), seed, _ptr(out), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "diffus_artifacts")
    return out, (dev, f, rad, loc, seed)


class _ArtifactsFn(torch.autograd.Function):
    """out = artifact chain(frames); backward via diffus_artifacts_bwd, which recomputes stages 1 and 2 from the
    frame, the noise and the seed the forward used."""

    @staticmethod
    def forward(ctx, frames, std_radial, std_local, max_sigma, alpha, seed, noise):
        out, (dev, f, rad, loc, seed) = _launch(frames, std_radial, std_local, max_sigma, alpha, seed, noise)
        ctx.launch = (dev, f, rad, loc, seed, float(std_radial), float(std_local), float(max_sigma), float(alpha))
        # nothing is stashed by value: the frame and the injected noise are read again by the backward, so their in-place
        # version counters are checked like autograd checks saved tensors (a private copy above is never touched again)
        ctx.versions = tuple((name, t, t._version) for name, t in (("frames", f), ("noise", rad), ("noise", loc))
                             if t is not None)
        ctx.meta = (frames.device, frames.dtype, tuple(frames.shape))
        out = out.reshape(frames.shape)
        return out if out.device == frames.device else out.to(frames.device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        lib = _lib.load()
        dev, f, rad, loc, seed, std_radial, std_local, max_sigma, alpha = ctx.launch
        for name, t, ver in ctx.versions:
            if t._version != ver:
                raise RuntimeError(f"diffus_amd: `{name}` was modified in place between the forward and this backward "
                                   f"(version {ver} -> {t._version}); the backward recomputes the forward from its inputs")
        fdev, fdt, fshape = ctx.meta
        P, R, N = f.shape
        with _Scope(dev):
            g = _as(gout, dev, torch.float64)
            gframe = torch.empty((P, R, N), dtype=torch.float64, device=dev)
            ws = _workspace(dev, lib.diffus_artifacts_bwd_workspace_bytes(P, R, N))
            rc = lib.diffus_artifacts_bwd(_ptr(f), P, R, N, std_radial, std_local, max_sigma, alpha, _ptr(rad), _ptr(loc),
                                          seed, _ptr(g), _ptr(gframe), _ptr(ws), ws.numel(), _stream(dev))
        _lib.check(rc, "diffus_artifacts_bwd")
        gframe = gframe.reshape(fshape)
        if gframe.device != fdev or gframe.dtype != fdt:
            gframe = gframe.to(device=fdev, dtype=fdt)
        return gframe, None, None, None, None, None, None


def apply_artifacts(frames: torch.Tensor, std_radial: float = 0.01, std_local: float = 0.15, max_sigma: float = 4.0,
                    alpha: float = 5, seed=None, noise=None) -> torch.Tensor:
    """frames (R,N) or (P,R,N) float32 -> same shape, float64, on frames.device.

    Differentiable in `frames` (not in the noise or the parameters); an auto-seeded call back-propagates through the
    draws it actually made."""
    if torch.is_grad_enabled() and frames.requires_grad:
        return _ArtifactsFn.apply(frames, std_radial, std_local, max_sigma, alpha, seed, noise)
    out, _ = _launch(frames, std_radial, std_local, max_sigma, alpha, seed, noise)
    out = out.reshape(frames.shape)
    return out if out.device == frames.device else out.to(frames.device)


def artifact_noise(shape, std_radial: float = 0.01, std_local: float = 0.15, seed: int = 0, device=None):
    """The speckle factors apply_artifacts(frames of `shape`, std_radial, std_local, seed=seed) multiplies by
    (diffus_artifacts_noise): -> (radial, local) float64, radial (N,) or (P,N), local of `shape` ((R,N) or (P,R,N)).
    Passed back as noise=(radial, local) they reproduce the seeded frame bit for bit."""
    lib = _lib.load()
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3):
        raise ValueError("shape must be (R, N) or (P, R, N)")
    P, R, N = (1,) + shape if len(shape) == 2 else shape
    dev = torch.device(device) if device is not None else _device_for(torch.empty(0))
    if dev.type != "cuda":
        raise _lib.DiffusError("artifact_noise draws on a HIP device; there is no CPU fallback")
    with _Scope(dev):
        radial = torch.empty((P, N), dtype=torch.float64, device=dev)
        local = torch.empty((P, R, N), dtype=torch.float64, device=dev)
        rc = lib.diffus_artifacts_noise(P, R, N, float(std_radial), float(std_local), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        _ptr(radial), _ptr(local), _stream(dev))
    _lib.check(rc, "diffus_artifacts_noise")
    if len(shape) == 2:
        return radial[0], local[0]
    return radial, local
