"""Host-side mirror of the reference's renderer API over the HIP C-ABI.

`UltrasoundRenderer` keeps the constructor and the `plot_beam_frame` signature,
argument meaning, return tuple and error behaviour of the reference
(src/renderer.py:18-25, :201-275), so `from diffus_amd import *` is a drop-in for
`from src.renderer import *` on this path.  All arithmetic happens in
libdiffus_hip.so (diffus_amd/csrc/*.hip); PyTorch only provides
device memory, the current HIP stream and autograd plumbing.  There is no CPU
fallback: without the built library every entry point raises DiffusError.

Differences from the reference, all deliberate:
  * no prints, no matplotlib figure per call (reference :122,179,245,252,:762-801);
  * `artifacts=True` (speckle arcs, lateral blur, unsharp mask, :264-273) runs on the GPU
    (diffus_artifacts) and, like the reference, returns float64; keyword-only `seed=` makes the
    speckle reproducible (the reference uses the unseeded global NumPy RNG);
  * extra keyword-only arguments `sampler=` ("nearest" = reference semantics,
    "trilinear" = differentiable in the pose) and `return_indices=`;
  * gradients work: d frame / d volume for both samplers, d / d source and
    d / d directions for trilinear (the reference raises);
  * a float `start` is honoured as the fraction of num_samples the code intends
    (:237-238); the reference crashes on it inside its visualisation (:774);
  * `render_poses` batches P poses in one launch;
  * `layout=` selects the HBM layout the kernels read: "canonical" (the caller's
    tensor), "bricked" / "paired" (cached converted copies, DESIGN.md §Data layout)
    or "auto" (= paired once a volume is used for a large or a second call); a
    `BrickedVolume` keeps a volume (e.g. a learnable impedance map) permanently
    bricked so that no conversion happens per step.
"""
from __future__ import annotations

import ctypes as C
import logging
import weakref
from typing import Optional

import torch

from . import _lib

log = logging.getLogger("diffus_amd")

_SAMPLERS = {"nearest": _lib.NEAREST, "prop": _lib.NEAREST, "trilinear": _lib.TRILINEAR}
_LAYOUTS = ("auto", "canonical", "bricked", "paired")
_workspaces: dict = {}
_gradbufs: dict = {}        # (device, shape) -> (bricked scratch, touched flags); all-zero between uses
_brick_cache: list = []     # [(weakref(source tensor), version, bricked copy)]   (at most 2 entries)
_brick_seen: list = []      # [(weakref(source tensor), version, calls)]
_AUTO_BRICK_SAMPLES = 1 << 18


class BrickedVolume:
    """A (d0,d1,d2) float32 volume stored in the bricked HBM layout.

    `data` is the flat bricked tensor (diffus_bricked_floats elements); it may
    require grad, in which case gradients come back in the same layout -- an
    optimiser can update it in place, element-wise, without ever converting.
    """

    def __init__(self, data: torch.Tensor, shape):
        self.data = data
        self.shape = tuple(int(x) for x in shape)

    @classmethod
    def from_dense(cls, volume: torch.Tensor) -> "BrickedVolume":
        return cls(brick_volume(volume), volume.shape)

    def to_dense(self) -> torch.Tensor:
        return unbrick_volume(self.data.detach(), self.shape)

    @property
    def device(self):
        return self.data.device


def _device_for(t: torch.Tensor) -> torch.device:
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise _lib.DiffusError("diffus_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# The drop-in path is HOST-bound (a 32-pose step is ~0.1 ms of kernels): what follows avoids torch/ctypes work that buys
# nothing per call -- the raw stream handle instead of a Stream object, plain ints for pointers (ctypes converts them to
# void* itself), no device context switch when the device is already current, no detach()/to()/contiguous() dispatches
# for tensors that are already what the kernels need.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_id(dev) -> int:
    """The current HIP stream of `dev` as an integer handle."""
    idx = dev.index
    if idx is None:
        idx = torch.cuda.current_device()
    if _raw_stream is not None:
        return _raw_stream(idx)
    return torch.cuda.current_stream(dev).cuda_stream


class _Scope:
    """`with _Scope(dev):` = torch.cuda.device(dev), skipped altogether when `dev` is already the current device."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        idx = dev.index
        cur = _cur_device() if _cur_device is not None else torch.cuda.current_device()
        self.ctx = None if (idx is None or idx == cur) else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            return self.ctx.__exit__(*a)


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """Scratch of the current stream of `dev` (one buffer per stream: two streams or autograd worker threads on one
    device never share contents).  A buffer that has to grow is replaced; the caching allocator hands the old block out
    again only to allocations of the same stream, i.e. behind the kernels still using it."""
    key = (dev, _stream_id(dev))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _workspaces[key] = ws
    return ws


_ws_bytes: dict = {}


def _render_ws_bytes(P: int, R: int, S: int, start: int) -> int:
    """diffus_workspace_bytes, remembered per shape (a ctypes round trip per call otherwise)."""
    key = (P, R, S, start)
    n = _ws_bytes.get(key)
    if n is None:
        if len(_ws_bytes) > 256:
            _ws_bytes.clear()
        n = _ws_bytes[key] = _lib.load().diffus_workspace_bytes(P, R, S, start)
    return n


def _gradbuf(dev: torch.device, shape):
    """Persistent sparse-gradient scratch of a device/shape/stream: bricked floats + one flag per brick.
    Invariant: both all-zero whenever no backward is in flight on that stream (diffus_gradbuf_flush restores it)."""
    stream = _stream_id(dev)
    key = (dev, tuple(shape), stream)   # one scratch per stream: no cross-stream races
    gb = _gradbufs.pop(key, None)
    if gb is None:
        lib = _lib.load()
        gb = (torch.zeros(lib.diffus_bricked_floats(*shape), dtype=torch.float32, device=dev),
              torch.zeros(lib.diffus_brick_count(*shape), dtype=torch.int32, device=dev))
        # evict the least recently used scratch OF THIS STREAM only: another stream's may have a flush in flight
        mine = [k for k in _gradbufs if k[0] == dev and k[2] == stream]
        if len(mine) >= 3:
            _gradbufs.pop(mine[0])
    _gradbufs[key] = gb                 # (re)inserted last: dict order = recency
    return gb


def _pose_dtype(t: torch.Tensor) -> torch.dtype:
    """torch promotion of `source + steps*directions` (reference :119-124):
    float64 stays float64, everything else computes in float32."""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _as(t: torch.Tensor, dev: torch.device, dtype: torch.dtype) -> torch.Tensor:
    """A tensor on `dev` of `dtype`, contiguous, for the kernels to READ (only its data pointer is used: no autograd
    history is created on it).  Already the case -- the usual one -- : the tensor itself, no dispatch at all."""
    if t.device == dev and t.dtype == dtype and t.is_contiguous():
        return t
    t = t.detach()
    if t.device != dev or t.dtype != dtype:
        t = t.to(device=dev, dtype=dtype)
    return t if t.is_contiguous() else t.contiguous()


# Small HOST tensors (the notebooks pass `source` and `directions` as CPU tensors, e.g. REUBEN DATA 46 cell 14): each
# `.to(device)` of pageable memory is a blocking ~15 us copy.  They go up together instead: packed into a slot of a pinned
# staging ring, ONE asynchronous copy into a fresh device buffer, typed views of that buffer.
_STAGE_SLOTS, _STAGE_BYTES = 8, 1 << 16
_staging: dict = {}


def _upload_small(dev: torch.device, items):
    """items: [(cpu tensor, dtype), ...] -> list of device tensors of those dtypes (same shapes), or None when the data is
    too large for a staging slot (the caller then converts one by one)."""
    sizes, total = [], 0
    for t, dt in items:
        nb = t.numel() * torch.empty((), dtype=dt).element_size()
        sizes.append((total, nb))
        total += (nb + 15) & ~15
    if total == 0 or total > _STAGE_BYTES:
        return None
    key = (dev, _stream_id(dev))
    st = _staging.get(key)
    if st is None:
        st = _staging[key] = {"buf": torch.empty((_STAGE_SLOTS, _STAGE_BYTES), dtype=torch.uint8).pin_memory(),
                              "ev": [None] * _STAGE_SLOTS, "next": 0}
    k = st["next"]
    st["next"] = (k + 1) % _STAGE_SLOTS
    if st["ev"][k] is not None:
        st["ev"][k].synchronize()            # the copy that last used this slot (eight uploads ago) has long finished
    slot = st["buf"][k]
    for (t, dt), (off, nb) in zip(items, sizes):
        if nb:
            slot[off:off + nb].view(dt).copy_(t.detach().reshape(-1))      # host-side cast + pack
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    out.copy_(slot[:total], non_blocking=True)
    ev = st["ev"][k] or torch.cuda.Event()
    ev.record()
    st["ev"][k] = ev
    return [out[off:off + nb].view(dt).reshape(t.shape) for (t, dt), (off, nb) in zip(items, sizes)]


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None        # ctypes turns the int into the void* of the signature


def _stream(dev) -> int:
    return _stream_id(dev)


def brick_volume(volume: torch.Tensor) -> torch.Tensor:
    """canonical (d0,d1,d2) -> flat bricked float32 tensor on the GPU (diffus_brick_volume)."""
    lib = _lib.load()
    dev = _device_for(volume)
    v = volume.detach().to(device=dev, dtype=torch.float32).contiguous()
    d0, d1, d2 = v.shape
    with _Scope(dev):
        out = torch.empty(lib.diffus_bricked_floats(d0, d1, d2), dtype=torch.float32, device=dev)
        rc = lib.diffus_brick_volume(_ptr(v), d0, d1, d2, _ptr(out), _stream(dev))
    _lib.check(rc, "diffus_brick_volume")
    return out


def pair_volume(volume: torch.Tensor) -> torch.Tensor:
    """canonical (d0,d1,d2) -> flat paired float32 tensor on the GPU (diffus_pair_volume)."""
    lib = _lib.load()
    dev = _device_for(volume)
    v = volume.detach().to(device=dev, dtype=torch.float32).contiguous()
    d0, d1, d2 = v.shape
    with _Scope(dev):
        out = torch.empty(lib.diffus_paired_floats(d0, d1, d2), dtype=torch.float32, device=dev)
        rc = lib.diffus_pair_volume(_ptr(v), d0, d1, d2, _ptr(out), _stream(dev))
    _lib.check(rc, "diffus_pair_volume")
    return out


def unbrick_volume(bricked: torch.Tensor, shape, out: Optional[torch.Tensor] = None, accumulate=False):
    """flat bricked tensor -> canonical (d0,d1,d2) float32 (diffus_unbrick_volume)."""
    lib = _lib.load()
    d0, d1, d2 = (int(x) for x in shape)
    dev = bricked.device
    with _Scope(dev):
        if out is None:
            out = torch.empty((d0, d1, d2), dtype=torch.float32, device=dev)
            accumulate = False
        rc = lib.diffus_unbrick_volume(_ptr(bricked), d0, d1, d2, _ptr(out), int(bool(accumulate)), _stream(dev))
    _lib.check(rc, "diffus_unbrick_volume")
    return out


def layout_fits(kind: str, shape) -> bool:
    """Whether a (d0,d1,d2) volume can be held in layout `kind` (include/diffus_hip.h, check_common): offsets are 32-bit
    (fewer than 2^30 floats) and the bricked / paired brick-row stride is the 24-bit operand of a multiply."""
    d0, d1, d2 = (int(x) for x in shape)
    nb0, nb1, nb2 = (d0 + 3) // 4, (d1 + 3) // 4, (d2 + 1) // 2
    if max(d0, d1, d2) > (1 << 24) or nb0 * nb1 * nb2 * 32 >= (1 << 30):
        return False
    if kind == "canonical":
        return True
    if kind == "bricked":
        return nb1 * nb2 * 128 < (1 << 24)
    if kind == "paired":
        return nb1 * d2 * 160 < (1 << 24) and nb0 * nb1 * d2 * 40 < (1 << 30)
    raise ValueError(f"unknown layout {kind!r}")


def _converted_copy(vol: torch.Tensor, src_tensor: torch.Tensor, want: str, samples: int):
    """Return (cached converted copy, layout id) if the layout policy asks for one, else (None, CANONICAL).

    Entries are keyed by the IDENTITY of the caller's tensor (weak reference), its in-place
    version counter and the layout -- never by address, which the allocator reuses.
    """
    if want == "canonical":
        return None, _lib.CANONICAL
    kind = "bricked" if want == "bricked" else "paired"
    if want == "auto" and not layout_fits(kind, vol.shape):     # very wide slices: fall back instead of failing
        kind = "bricked" if layout_fits("bricked", vol.shape) else None
        if kind is None:
            return None, _lib.CANONICAL
    lid = _lib.BRICKED if kind == "bricked" else _lib.PAIRED
    ver = src_tensor._version
    _brick_cache[:] = [e for e in _brick_cache if e[0]() is not None]
    for ref, v, k, b in _brick_cache:
        if ref() is src_tensor and v == ver and k == kind:
            return b, lid
    _brick_seen[:] = [e for e in _brick_seen if e[0]() is not None][-16:]
    calls = 1
    for i, (ref, v, n) in enumerate(_brick_seen):
        if ref() is src_tensor and v == ver:
            calls = n + 1
            _brick_seen[i] = (ref, v, calls)
            break
    else:
        _brick_seen.append((weakref.ref(src_tensor), ver, 1))
    if want == "auto" and samples < _AUTO_BRICK_SAMPLES and calls < 2:
        return None, _lib.CANONICAL
    b = brick_volume(vol) if kind == "bricked" else pair_volume(vol)
    _brick_cache.append((weakref.ref(src_tensor), ver, kind, b))
    del _brick_cache[:-2]
    return b, lid


def resolve_start(start, num_samples: int) -> int:
    """reference src/renderer.py:237-240."""
    if type(start) is float:
        start = int(start * num_samples)
    if type(start) is int:
        start = max(0, start)
    return int(start)


# Host poses already uploaded: (weakref source, version, weakref directions, version, device) -> (device source, device
# directions, planar).  The reference's notebooks build `source` / `directions` once on the host and call plot_beam_frame in a
# loop (REUBEN DATA 46 cell 14): packing, the pinned copy and its event were 45 us of an 85 us call.  The device copies are only
# ever READ by the kernels; an in-place edit of a host tensor bumps its version and misses.
_host_poses: list = []

try:
    from xxhash import xxh3_64_intdigest as _digest          # ~10 GB/s: 3 KB of directions in well under a microsecond
except Exception:                                            # pragma: no cover
    from zlib import adler32 as _digest


def _fingerprint(t: torch.Tensor) -> int:
    """A checksum of a host tensor's bytes.  The version counter does not see every edit: a tensor made by torch.from_numpy
    shares its memory with an array that NumPy code may rewrite in place -- the cached device copy would then be stale
    without any sign of it.  So a hit needs identity, version AND content."""
    return _digest(t.numpy() if t.is_contiguous() else t.contiguous().numpy())      # (callers: host tensors that do not require grad)


def _host_pose_lookup(dev, sources, directions):
    if sources.requires_grad or directions.requires_grad:
        return None
    for e in _host_poses:
        if e[0]() is sources and e[2]() is directions and e[1] == sources._version and e[3] == directions._version and e[4] == dev:
            if e[8] == (_fingerprint(sources), _fingerprint(directions)):
                return e[5], e[6], e[7]
            return None
    return None


def _host_pose_store(dev, sources, directions, dsrc, ddirs, planar):
    if sources.requires_grad or directions.requires_grad:
        return
    _host_poses[:] = [e for e in _host_poses if e[0]() is not None and e[2]() is not None
                      and not (e[0]() is sources and e[2]() is directions and e[4] == dev)][-7:]
    _host_poses.append((weakref.ref(sources), sources._version, weakref.ref(directions), directions._version, dev, dsrc, ddirs, planar,
                        (_fingerprint(sources), _fingerprint(directions))))


_planar_seen: list = []          # (weakref to a device `directions` tensor, version, planar): one readback per tensor version


def _fans_planar(directions: torch.Tensor):
    """Whether NO direction moves along dim 2 (every fan of the reference: src/cone.py:258) -- the hint that selects the
    scatter launch for planar fans (DIFFUS_FANS_PLANAR).  Host tensors are looked at directly; a device tensor that is not
    being optimised costs one readback per tensor version; directions that require grad (a pose optimisation changes them
    every step, and tilts them) stay unknown (None): the launch that also carries the slab path."""
    if directions.shape[-1] != 3:
        return None
    if getattr(directions, "_diffus_planar", False):      # set by FanPose for an in-plane fan (exact zeros by construction)
        return True
    if not directions.is_cuda:
        return bool((directions.detach()[..., 2] == 0).all())
    if directions.requires_grad or directions.grad_fn is not None:
        return None
    _planar_seen[:] = [e for e in _planar_seen if e[0]() is not None][-8:]
    for ref, ver, val in _planar_seen:
        if ref() is directions and ver == directions._version:
            return val
    val = bool((directions[..., 2] == 0).all())
    _planar_seen.append((weakref.ref(directions), directions._version, val))
    return val


def _sources_level(sources: torch.Tensor):
    """Per-ray sources (P,R,3): whether every pose's origins share one dim-2 coordinate -- with directions that do not move
    along dim 2, the array then lies in one slice and the planar-fan hint holds.  Same rules as _fans_planar: host tensors
    are looked at, a device tensor that is not being optimised costs one readback, one that requires grad is unknown
    (None) unless ArrayPose marked it."""
    if getattr(sources, "_diffus_planar", False):
        return True
    if sources.is_cuda and (sources.requires_grad or sources.grad_fn is not None):
        return None
    s = sources.detach()[..., 2]
    return bool((s == s[..., :1]).all())


class _Problem:
    """Validated, device-resident arguments of one (batched) call.  `sources` (P,3) or (3,): one apex per pose;
    (P,R,3): one origin per ray (DIFFUS_SRC_PER_RAY) -- a 3-D `sources` is the only thing that selects that form."""

    def __init__(self, volume, sources, directions, S, start, alpha, sampler, layout="auto", shape=None):
        if layout not in _LAYOUTS + ("prebricked",):
            raise ValueError(f"unknown layout {layout!r}")
        if layout == "prebricked":          # `volume` is BrickedVolume.data, `shape` its dense shape
            self.dev = _device_for(volume)
            self.shape = tuple(shape)
            self.vol = None
            self.bricked = _as(volume, self.dev, torch.float32)
        else:
            if volume.dim() != 3:
                raise ValueError(f"volume must be 3-D, got shape {tuple(volume.shape)}")
            self.dev = _device_for(volume)
            self.shape = tuple(volume.shape)
            self.vol = _as(volume, self.dev, torch.float32)
            self.bricked = None
        self._layout_req, self._vol_src = layout, volume
        self._common = None
        sd, dd = _pose_dtype(sources), _pose_dtype(directions)
        self.per_ray = sources.dim() == 3
        if self.per_ray and (sources.shape[-1] != 3 or directions.shape[-1] != 3 or directions.dim() not in (2, 3)
                             or directions.shape[-2] != sources.shape[1]
                             or (directions.dim() == 3 and directions.shape[0] != sources.shape[0])):
            raise ValueError(f"per-ray sources (P,R,3) need directions (R,3) or (P,R,3) with the same R; got sources "
                             f"{tuple(sources.shape)}, directions {tuple(directions.shape)}")

        def planar_hint(srcs, dirs):
            p = _fans_planar(dirs)
            return (p and _sources_level(srcs)) if self.per_ray else p

        if not sources.is_cuda and not directions.is_cuda:       # host poses: one packed, asynchronous upload ...
            hit = _host_pose_lookup(self.dev, sources, directions)
            if hit is not None:                                  # ... once per (tensor, version): a notebook renders the same fan again
                sources, directions, self.planar = hit
            else:
                self.planar = planar_hint(sources, directions)
                with _Scope(self.dev):
                    up = _upload_small(self.dev, [(sources, sd), (directions, dd)])
                if up is not None:
                    _host_pose_store(self.dev, sources, directions, up[0], up[1], self.planar)
                    sources, directions = up
        else:
            self.planar = planar_hint(sources, directions)
        self.src = _as(sources, self.dev, sd)
        if not self.per_ray and (self.src.dim() != 2 or self.src.shape[1] != 3):
            self.src = self.src.reshape(-1, 3)
            if not self.src.is_contiguous():
                self.src = self.src.contiguous()
        d = _as(directions, self.dev, dd)
        if d.dim() == 1:
            d = d.unsqueeze(0)
        self.P = self.src.shape[0]
        if d.dim() == 2:
            d = d.unsqueeze(0).expand(self.P, -1, -1)
        if d.dim() != 3 or d.shape[0] != self.P or d.shape[-1] != 3:
            raise ValueError(f"directions must be (R,3) or (P,R,3); got {tuple(directions.shape)} for P={self.P}")
        self.dirs = d if d.is_contiguous() else d.contiguous()
        self.R = self.dirs.shape[1]
        self.S, self.start, self.alpha = int(S), int(start), float(alpha)
        self.N1 = self.S - self.start
        self.sampler = _SAMPLERS[sampler]
        self.src_dt = (_lib.DIFFUS_F64 if sd == torch.float64 else _lib.DIFFUS_F32) | (_lib.SRC_PER_RAY if self.per_ray else 0)
        self.dir_dt = _lib.DIFFUS_F64 if dd == torch.float64 else _lib.DIFFUS_F32
        if self.bricked is None:
            self.bricked, self.layout = _converted_copy(self.vol, volume, layout, self.P * self.R * self.N1)
        else:
            self.layout = _lib.BRICKED

    def common(self):
        c = self._common
        if c is None:
            d0, d1, d2 = self.shape
            v = self.bricked if self.layout != _lib.CANONICAL else self.vol
            c = self._common = (_ptr(v), d0, d1, d2, self.layout, _ptr(self.src), self.src_dt, _ptr(self.dirs), self.dir_dt,
                                self.P, self.R, self.S, self.start, self.alpha, self.sampler)
        return c

    def common_bwd(self):
        """common() for the backward entry points: the layout word also carries the planar-fan hint."""
        c = self.common()
        return c[:4] + (c[4] | _lib.FANS_PLANAR,) + c[5:] if self.planar else c

    def workspace(self):
        return _workspace(self.dev, _render_ws_bytes(self.P, self.R, self.S, self.start))


def _forward_launch(pb: "_Problem", want_idx: bool, squeeze_pose: bool = False):
    """diffus_render_fwd on a validated problem -> (frame (P,R,N1), idx (3,P,R,N1) or None); squeeze_pose (P == 1): the same
    buffers shaped (R,N1) / (3,R,N1), so that a one-pose caller needs no indexing ops afterwards."""
    lib = _lib.load()
    with _Scope(pb.dev):
        one = squeeze_pose and pb.P == 1
        frame = torch.empty((pb.R, pb.N1) if one else (pb.P, pb.R, pb.N1), dtype=torch.float32, device=pb.dev)
        idx = (torch.empty((3, pb.R, pb.N1) if one else (3, pb.P, pb.R, pb.N1), dtype=torch.int64, device=pb.dev)
               if want_idx else None)
        ws = pb.workspace()
        rc = lib.diffus_render_fwd(*pb.common(), _ptr(frame), _ptr(idx), _ptr(ws), ws.numel(), _stream(pb.dev))
    _lib.check(rc, "diffus_render_fwd")
    return frame, idx


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _aliased_versions(pb: "_Problem", volume, sources, directions):
    """The backward recomputes the forward from the tensors as they are THEN (nothing is stashed by value): it is only
    right if they are unchanged, so their in-place version counters are checked like autograd checks saved tensors.
    Checked only for the inputs the kernels will actually READ AGAIN through the caller's storage: a private copy made
    by _Problem (device / dtype conversion, the cached bricked or paired volume) keeps the forward's values whatever the
    caller does to the original afterwards.  -> ((name, tensor, version), ...) for _check_versions."""
    reads_vol = pb.vol is not None and pb.layout == _lib.CANONICAL and pb.vol.data_ptr() == volume.data_ptr()
    reads_bricked = pb.vol is None and pb.bricked.data_ptr() == volume.data_ptr()          # a BrickedVolume's own data
    return tuple((name, t, t._version) for name, t, aliased in (
        ("volume", volume, reads_vol or reads_bricked),
        ("sources", sources, pb.src.data_ptr() == sources.data_ptr()),
        ("directions", directions, pb.dirs.data_ptr() == directions.data_ptr())) if aliased)


def _check_versions(versions):
    for name, t, ver in versions:
        if t._version != ver:
            raise RuntimeError(f"diffus_amd: `{name}` was modified in place between the forward and this backward "
                               f"(version {ver} -> {t._version}); the backward recomputes the forward from its inputs")


def _pose_meta(volume, sources, directions):
    return (volume.device, volume.dtype, sources.device, sources.dtype, tuple(sources.shape),
            directions.device, directions.dtype, tuple(directions.shape))


def _pose_grads(meta, gsrc, gdirs):
    """(P,3) / (P,R,3) float32 pose gradients (None: not wanted) -> the caller's shapes, devices and dtypes; a fan
    shared by all poses gets the sum over the poses."""
    _, _, sdev, sdt, sshape, ddev, ddt, dshape = meta
    out_s = None
    if gsrc is not None:
        out_s = gsrc.reshape(sshape)
        if out_s.device != sdev or out_s.dtype != sdt:
            out_s = out_s.to(device=sdev, dtype=sdt)
    out_d = None
    if gdirs is not None:
        if len(dshape) == 3:
            out_d = gdirs
        elif len(dshape) == 2:      # one fan shared by all poses
            out_d = gdirs.sum(0)
        else:
            out_d = gdirs.sum(0).reshape(dshape)
        if out_d.device != ddev or out_d.dtype != ddt:
            out_d = out_d.to(device=ddev, dtype=ddt)
    return out_s, out_d


class _RenderFn(torch.autograd.Function):
    """frame = render(volume, sources, directions); backward via diffus_render_bwd."""

    @staticmethod
    def forward(ctx, volume, sources, directions, S, start, alpha, sampler, want_idx, layout, shape):
        pb = _Problem(volume, sources, directions, S, start, alpha, sampler, layout, shape)
        frame, idx = _forward_launch(pb, want_idx)
        ctx.pb = pb
        ctx.versions = _aliased_versions(pb, volume, sources, directions)
        ctx.meta = _pose_meta(volume, sources, directions)
        if idx is None:
            idx = torch.empty(0, dtype=torch.int64, device=pb.dev)
        ctx.mark_non_differentiable(idx)
        return frame, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gframe, _gidx):
        lib = _lib.load()
        pb = ctx.pb
        _check_versions(ctx.versions)
        vdev, vdt = ctx.meta[:2]
        need_v, need_s, need_d = ctx.needs_input_grad[:3]
        with _Scope(pb.dev):
            g = _as(gframe, pb.dev, torch.float32)
            gvol = touched = None
            sparse = False
            common = pb.common_bwd()
            if need_v:      # gradient buffer in the layout that goes with the volume's
                if pb.layout == _lib.CANONICAL and layout_fits("bricked", pb.shape):
                    # a canonical volume's gradient goes through the BRICKED scratch too (DIFFUS_GRAD_BRICKED): its scatter
                    # accumulates planar and tilted fans in doubles, where the canonical tile is 32-bit fixed point with one scale
                    # per patch -- 7e-3 off on 0.04-voxel steps whose contributions cancel (tools/fuzz_one_pass.py, seed 55) --
                    # and the dense hand-back below costs what zeroing a canonical gradient would
                    gvol, touched = _gradbuf(pb.dev, pb.shape)
                    sparse = True
                    common = common[:4] + (common[4] | _lib.GRAD_BRICKED,) + common[5:]
                elif pb.layout == _lib.CANONICAL:
                    gvol = torch.zeros_like(pb.vol)
                elif pb._layout_req == "prebricked":
                    gvol = torch.zeros(lib.diffus_bricked_floats(*pb.shape), dtype=torch.float32, device=pb.dev)
                else:       # sparse: persistent all-zero scratch + touched flags, flushed below
                    gvol, touched = _gradbuf(pb.dev, pb.shape)
                    sparse = True
            gsrc = torch.empty(pb.src.shape, dtype=torch.float32, device=pb.dev) if need_s else None
            gdirs = torch.empty((pb.P, pb.R, 3), dtype=torch.float32, device=pb.dev) if need_d else None
            ws = pb.workspace()
            rc = lib.diffus_render_bwd(*common, _ptr(g), _ptr(gvol), _ptr(touched), _ptr(gsrc), _ptr(gdirs),
                                       _lib.BWD_ALL, _ptr(ws), ws.numel(), _stream(pb.dev))
            _lib.check(rc, "diffus_render_bwd")
            if sparse:      # a fresh dense (d0,d1,d2) gradient in ONE launch: touched bricks' values, zeros elsewhere
                dense = torch.empty(pb.shape, dtype=torch.float32, device=pb.dev)
                rc = lib.diffus_gradbuf_flush(_ptr(gvol), _ptr(touched), *pb.shape, _ptr(dense), _lib.FLUSH_DENSE, _stream(pb.dev))
                _lib.check(rc, "diffus_gradbuf_flush")
                gvol = dense
        out_v = (gvol if (gvol.device == vdev and gvol.dtype == vdt) else gvol.to(device=vdev, dtype=vdt)) if need_v else None
        out_s, out_d = _pose_grads(ctx.meta, gsrc, gdirs)
        return out_v, out_s, out_d, None, None, None, None, None, None, None


def render_poses(volume, sources, directions, num_samples, attenuation_coeff, start=0, sampler="nearest",
                 return_indices=False, layout="auto", _squeeze_pose=False):
    """Batched hot path: P poses in one launch.

    volume (d0,d1,d2) tensor or BrickedVolume; sources (P,3) or (3,): one apex per pose (sector fans), or (P,R,3): one
    origin per ray (linear and convex arrays, see diffus_amd.probes); directions (P,R,3) or (R,3) shared.
    -> frame (P,R,num_samples-start) float32 [, idx (3,P,R,N1) int64].  d/dsources has the shape of `sources`.
    Differentiable in volume (both samplers) and in sources/directions (trilinear).
    """
    if sampler not in _SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}")
    start = resolve_start(start, num_samples)
    if start > 0 and start >= num_samples - 1:
        raise IndexError("index 0 is out of bounds for dimension 1 with size 0")  # reference :243
    if not _wants_grad(volume.data if isinstance(volume, BrickedVolume) else volume, sources, directions):
        # nothing to differentiate (the notebooks' rendering loops): straight to the launch, no autograd node (~10 us of host time)
        if isinstance(volume, BrickedVolume):
            pb = _Problem(volume.data, sources, directions, num_samples, start, attenuation_coeff, sampler, "prebricked", volume.shape)
        else:
            pb = _Problem(volume, sources, directions, num_samples, start, attenuation_coeff, sampler, layout, None)
        frame, idx = _forward_launch(pb, bool(return_indices), squeeze_pose=_squeeze_pose)
        return (frame, idx) if return_indices else frame
    if isinstance(volume, BrickedVolume):
        frame, idx = _RenderFn.apply(volume.data, sources, directions, num_samples, start, attenuation_coeff,
                                     sampler, bool(return_indices), "prebricked", volume.shape)
    else:
        frame, idx = _RenderFn.apply(volume, sources, directions, num_samples, start, attenuation_coeff,
                                     sampler, bool(return_indices), layout, None)
    return (frame, idx) if return_indices else frame


def _trace_launch(pb: "_Problem", want):
    """diffus_trace_rays on a validated problem -> (imp, refl, idx), None where not in `want`."""
    lib = _lib.load()
    with _Scope(pb.dev):
        imp = torch.empty((pb.P, pb.R, pb.S), dtype=torch.float32, device=pb.dev) if "imp" in want else None
        refl = torch.empty((pb.P, pb.R, pb.S - 1), dtype=torch.float32, device=pb.dev) if "refl" in want else None
        idx = torch.empty((3, pb.P, pb.R, pb.S), dtype=torch.int64, device=pb.dev) if "idx" in want else None
        c = pb.common()
        rc = lib.diffus_trace_rays(*c[:12], pb.sampler, _ptr(imp), _ptr(refl), _ptr(idx), _stream(pb.dev))
    _lib.check(rc, "diffus_trace_rays")
    return imp, refl, idx


class _TraceFn(torch.autograd.Function):
    """(imp, refl, idx) = trace_rays(volume, sources, directions); backward via diffus_trace_rays_bwd, which samples the
    volume again from the same (possibly converted) copy the forward read.  Outputs not asked for are empty tensors."""

    @staticmethod
    def forward(ctx, volume, sources, directions, S, sampler, want, layout):
        pb = _Problem(volume, sources, directions, S, 0, 0.0, sampler, layout)
        imp, refl, idx = _trace_launch(pb, want)
        ctx.pb = pb
        ctx.versions = _aliased_versions(pb, volume, sources, directions)
        ctx.meta = _pose_meta(volume, sources, directions)
        ctx.set_materialize_grads(False)
        empty = torch.empty(0, dtype=torch.float32, device=pb.dev)
        idx = torch.empty(0, dtype=torch.int64, device=pb.dev) if idx is None else idx
        ctx.mark_non_differentiable(idx)
        return (empty if imp is None else imp), (empty if refl is None else refl), idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gimp, grefl, _gidx):
        lib = _lib.load()
        pb = ctx.pb
        _check_versions(ctx.versions)
        vdev, vdt = ctx.meta[:2]
        need_v, need_s, need_d = ctx.needs_input_grad[:3]
        with _Scope(pb.dev):
            gi = _as(gimp, pb.dev, torch.float32) if gimp is not None and gimp.numel() else None
            gr = _as(grefl, pb.dev, torch.float32) if grefl is not None and grefl.numel() else None
            gvol = torch.zeros(pb.shape, dtype=torch.float32, device=pb.dev) if need_v else None
            gsrc = torch.empty(pb.src.shape, dtype=torch.float32, device=pb.dev) if need_s else None
            gdirs = torch.empty((pb.P, pb.R, 3), dtype=torch.float32, device=pb.dev) if need_d else None
            nws = lib.diffus_trace_rays_bwd_workspace_bytes(pb.P, pb.R) if need_s else 0
            ws = torch.empty(nws, dtype=torch.uint8, device=pb.dev) if nws else None
            c = pb.common()
            rc = lib.diffus_trace_rays_bwd(*c[:12], pb.sampler, _ptr(gi), _ptr(gr), _ptr(gvol), _ptr(gsrc), _ptr(gdirs),
                                           _ptr(ws), nws, _stream(pb.dev))
        _lib.check(rc, "diffus_trace_rays_bwd")
        out_v = (gvol if (gvol.device == vdev and gvol.dtype == vdt) else gvol.to(device=vdev, dtype=vdt)) if need_v else None
        out_s, out_d = _pose_grads(ctx.meta, gsrc, gdirs)
        return out_v, out_s, out_d, None, None, None, None


def trace_rays(volume, sources, directions, num_samples, sampler="nearest", want=("imp", "refl", "idx"),
               layout="auto"):
    """Stage 1 alone (diffus_trace_rays): -> dict with imp (P,R,S), refl (P,R,S-1), idx (3,P,R,S) (None where not in
    `want`).  `sources` as in render_poses: (P,3) / (3,) one apex per pose, (P,R,3) one origin per ray.
    Differentiable in volume (both samplers) and in sources/directions (trilinear; nearest gives them zeros,
    as render_poses does) through diffus_trace_rays_bwd."""
    if not _wants_grad(volume, sources, directions):
        pb = _Problem(volume, sources, directions, num_samples, 0, 0.0, sampler, layout)
        imp, refl, idx = _trace_launch(pb, want)
    else:
        imp, refl, idx = _TraceFn.apply(volume, sources, directions, num_samples, sampler, tuple(want), layout)
        imp = imp if "imp" in want else None
        refl = refl if "refl" in want else None
        idx = idx if "idx" in want else None
    return {"imp": imp, "refl": refl, "idx": idx}


class _EchoFn(torch.autograd.Function):
    """echo = diffus_echo_traces(r); backward = diffus_echo_traces_bwd (the O(N) adjoint of SURVEY App. A.4) -- what torch
    autograd does through the reference's N+1 linalg.solve nodes (src/renderer.py:407,430,454).  `cumulate`: the running
    sum of propagate_full_rays_batched (:435) on top (its adjoint is a reversed running sum of the incoming gradient)."""

    @staticmethod
    def forward(ctx, refLR, cumulate):
        lib = _lib.load()
        dev = _device_for(refLR)
        r = _as(refLR, dev, torch.float32)
        B, N = r.shape
        with _Scope(dev):
            out = torch.empty((B, N + 1), dtype=torch.float32, device=dev)
            if B:
                fn, name = (lib.diffus_propagate_rays, "diffus_propagate_rays") if cumulate else (lib.diffus_echo_traces, "diffus_echo_traces")
                _lib.check(fn(_ptr(r) if N else None, B, N, _ptr(out), _stream(dev)), name)
        ctx.save_for_backward(r)           # torch raises if refLR is edited in place before the backward
        ctx.cumulate = bool(cumulate)
        ctx.meta = (refLR.device, refLR.dtype if refLR.is_floating_point() else torch.float32)
        return out.to(device=ctx.meta[0], dtype=ctx.meta[1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        lib = _lib.load()
        r, = ctx.saved_tensors
        dev = r.device
        B, N = r.shape
        g = _as(gout, dev, torch.float32)
        if ctx.cumulate:            # d/d echo_n = sum over m >= n of d/d cum_m
            g = torch.flip(torch.cumsum(torch.flip(g, (1,)), 1), (1,)).contiguous()
        with _Scope(dev):
            gr = torch.zeros((B, N), dtype=torch.float32, device=dev)
            if B and N:
                nws = lib.diffus_echo_bwd_workspace_bytes(B, N)
                ws = torch.empty(nws, dtype=torch.uint8, device=dev)    # own buffer: (N+1) x B x 36 bytes can be large
                _lib.check(lib.diffus_echo_traces_bwd(_ptr(r), B, N, _ptr(g), _ptr(gr), _ptr(ws), ws.numel(), _stream(dev)),
                           "diffus_echo_traces_bwd")
        return gr.to(device=ctx.meta[0], dtype=ctx.meta[1]), None


def compute_echo_traces(refLR: torch.Tensor, spacing: float = 1.0, c: float = 1.54e3):
    """Mirror of reference src/renderer.py:439-457: (echo_signals (B,N+1), delays_us (N+1,)).  Differentiable in refLR
    like the reference's (diffus_echo_traces_bwd: the O(N) adjoint instead of N+1 LinalgSolveBackward nodes)."""
    if refLR.dim() != 2:
        raise ValueError("not enough values to unpack (expected 2, got %d)" % refLR.dim())  # B, N = refLR.shape
    N = refLR.shape[1]
    echo = _EchoFn.apply(refLR, False)
    delays_us = 2 * spacing * torch.arange(N + 1, device=refLR.device) / c
    return echo, delays_us


def prop_single_ray(refLR: torch.Tensor, traLR: torch.Tensor = None, traRL: torch.Tensor = None) -> torch.Tensor:
    """Mirror of reference src/renderer.py:367-410: refLR (B,N) -> w (B, 2(N+1)) = [g0,d0,...,gN,dN], the solution of
    the dense interface system of every ray -- evaluated in closed form on the GPU (diffus_prop_single_ray) instead of
    torch.linalg.solve.  `traLR` / `traRL` are accepted and ignored, as in the reference (:380-381 overwrite them).

    Two differences from the reference, both loud or documented: (1) the FULL solution vector has no backward here --
    a `refLR` that requires grad raises instead of silently returning a tensor without grad_fn (the echo series, i.e.
    w[:, 1] of every truncation, IS differentiable: compute_echo_traces / propagate_full_rays_batched);  (2) the
    reference's nan_to_num(nan=0.0) (:408) maps +-inf entries of a solved system to +-float max, this closed form
    returns an all-zero row whenever a coefficient is non-finite (the reference's LU then yields NaN -> 0 everywhere as
    well; only an overflow INSIDE a solve with finite coefficients would differ)."""
    lib = _lib.load()
    if refLR.dim() != 2:
        raise ValueError("not enough values to unpack (expected 2, got %d)" % refLR.dim())  # B, N = refLR.shape
    if refLR.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("diffus_amd.prop_single_ray has no backward for the full solution vector; use "
                                  "compute_echo_traces / propagate_full_rays_batched (differentiable) or detach refLR")
    dev = _device_for(refLR)
    dt = torch.float64 if refLR.dtype == torch.float64 else torch.float32
    r = _as(refLR, dev, dt)
    B, N = r.shape
    with _Scope(dev):
        w = torch.empty((B, 2 * (N + 1)), dtype=dt, device=dev)
        if B:
            rc = lib.diffus_prop_single_ray(_ptr(r) if N else None, _lib.DIFFUS_F64 if dt == torch.float64 else _lib.DIFFUS_F32,
                                            B, N, _ptr(w), _stream(dev))
            _lib.check(rc, "diffus_prop_single_ray")
    return w.to(device=refLR.device, dtype=refLR.dtype if refLR.is_floating_point() else torch.float32)


def propagate_full_rays_batched(refLR: torch.Tensor) -> torch.Tensor:
    """Mirror of reference src/renderer.py:412-436: refLR (B,N) -> (B,N+1), the surface return d0 of every truncation
    depth, cumulated along the depth (diffus_propagate_rays: the O(N) echo series + a running sum).  Differentiable in
    refLR like the reference's."""
    if refLR.dim() != 2:
        raise ValueError("not enough values to unpack (expected 2, got %d)" % refLR.dim())
    return _EchoFn.apply(refLR, True)


def custom_nearest_sampler(Z: torch.Tensor, points: torch.Tensor, visualize: bool = True, sampler: str = "prop",
                           start: int = 100):
    """Mirror of reference src/renderer.py:741-819 for the default sampler 'prop': points (batch, num_samples, 3) in
    voxel coordinates -> (x, y, z, ray_values), each (batch, num_samples); indices are rounded half to even and
    clamped into the volume (:754-756).  `visualize` and `start` only drive the reference's matplotlib figure
    (:762-801), which is not reproduced: they are accepted and ignored.  Differentiable in Z (both samplers) and in
    points (trilinear) through diffus_sample_points_bwd; under nearest the points get no gradient, as in the reference."""
    _lib.load()
    if sampler not in _SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}")
    if Z.dim() != 3:
        raise ValueError("not enough values to unpack (expected 3, got %d)" % Z.dim())       # D, H, W = Z.shape
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"points must be (batch, num_samples, 3); got {tuple(points.shape)}")
    tri = _SAMPLERS[sampler] == _lib.TRILINEAR
    if _wants_grad(Z) or (tri and _wants_grad(points)):  # nearest: the reference's .round().long() cuts the points' graph
        vals, idx = _SampleFn.apply(Z, points, sampler)
        return idx[0], idx[1], idx[2], vals
    _, _, val, idx = _sample_launch(Z, points, sampler)
    out_dev = Z.device
    vals = val.to(device=out_dev, dtype=Z.dtype if Z.is_floating_point() else torch.float32)
    return idx[0].to(out_dev), idx[1].to(out_dev), idx[2].to(out_dev), vals


def _sample_launch(Z, points, sampler):
    """diffus_sample_points -> (device volume, device points (b,ns,3) float32, values (b,ns), idx (3,b,ns)) on the GPU."""
    lib = _lib.load()
    dev = _device_for(Z)
    vol = _as(Z, dev, torch.float32)
    pts = _as(points, dev, torch.float32)            # the reference's `points.float()` (:751)
    b, ns, _ = pts.shape
    n = b * ns
    d0, d1, d2 = vol.shape
    with _Scope(dev):
        val = torch.empty((b, ns), dtype=torch.float32, device=dev)
        idx = torch.empty((3, b, ns), dtype=torch.int64, device=dev)
        if n:
            rc = lib.diffus_sample_points(_ptr(vol), d0, d1, d2, _lib.CANONICAL, _ptr(pts), n, _SAMPLERS[sampler], _ptr(val),
                                          _ptr(idx), _stream(dev))
            _lib.check(rc, "diffus_sample_points")
    return vol, pts, val, idx


class _SampleFn(torch.autograd.Function):
    """(values, idx) = custom_nearest_sampler(Z, points); backward via diffus_sample_points_bwd: d/d Z for both samplers,
    d/d points for trilinear (None for nearest, as in the reference's graph)."""

    @staticmethod
    def forward(ctx, Z, points, sampler):
        vol, pts, val, idx = _sample_launch(Z, points, sampler)
        ctx.bufs = (vol, pts)
        ctx.sampler = _SAMPLERS[sampler]
        # the backward reads the volume and the points again: see _aliased_versions
        ctx.versions = tuple((name, t, t._version) for name, t, buf in (("Z", Z, vol), ("points", points, pts))
                             if buf.data_ptr() == t.data_ptr())
        ctx.meta = (Z.device, Z.dtype, points.device, points.dtype)
        out_dev = Z.device
        idx = idx.to(out_dev)
        ctx.mark_non_differentiable(idx)
        return val.to(device=out_dev, dtype=Z.dtype if Z.is_floating_point() else torch.float32), idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gvals, _gidx):
        lib = _lib.load()
        _check_versions(ctx.versions)
        vol, pts = ctx.bufs
        zdev, zdt, pdev, pdt = ctx.meta
        need_z = ctx.needs_input_grad[0]
        need_p = ctx.needs_input_grad[1] and ctx.sampler == _lib.TRILINEAR
        dev = vol.device
        n = pts.shape[0] * pts.shape[1]
        with _Scope(dev):
            gz = torch.zeros(vol.shape, dtype=torch.float32, device=dev) if need_z else None
            gp = torch.zeros(pts.shape, dtype=torch.float32, device=dev) if need_p else None
            if n and (need_z or need_p):
                g = _as(gvals, dev, torch.float32)
                rc = lib.diffus_sample_points_bwd(_ptr(vol), *vol.shape, _lib.CANONICAL, _ptr(pts), n, ctx.sampler, _ptr(g),
                                                  _ptr(gz), _ptr(gp), _stream(dev))
                _lib.check(rc, "diffus_sample_points_bwd")
        out_z = gz.to(device=zdev, dtype=zdt) if need_z else None
        out_p = gp.to(device=pdev, dtype=pdt) if need_p else None
        return out_z, out_p, None


def gaussian_pulse(length: int, sigma: float):
    """Gaussian pulse of `length` taps on the grid linspace(-length // 2, length // 2), peak normalised to 1
    (what reference src/renderer.py:481-496 returns; NumPy float64, host side)."""
    import numpy as np
    grid = np.linspace(-length // 2, length // 2, length)
    g = np.exp(-0.5 * (grid / sigma) ** 2)
    return g / g.max()


def compute_gaussian_pulse(refLR: torch.Tensor, spacing: float = 1.0, c: float = 1.54e3, length: int = 10,
                           sigma: int = 1, pulse=None) -> torch.Tensor:
    """Echo series of every ray passed through the transducer pulse (reference src/renderer.py:459-479): echo traces
    by diffus_echo_traces, then each row correlated with the pulse (`length` taps, `length // 2` zeros of padding on
    both sides, like the F.conv1d at :477) by diffus_rows_conv1d.  `pulse` may be given as a (1,1,L) tensor like the
    reference's; the default is gaussian_pulse(length, sigma).  Differentiable in refLR and in a `pulse` tensor
    (diffus_echo_traces_bwd, diffus_rows_conv1d_bwd)."""
    _lib.load()
    echo, _ = compute_echo_traces(refLR, spacing, c)
    taps = gaussian_pulse(length=length, sigma=sigma) if pulse is None else pulse
    if _wants_grad(echo, taps):
        return _PulseFn.apply(echo, taps, length // 2)
    return _pulse_launch(echo, taps, length // 2)[0]


def _pulse_launch(echo, taps, pad):
    """diffus_rows_conv1d of every echo row with the taps -> (out on echo's device, device echo, device taps)."""
    lib = _lib.load()
    dev = echo.device if echo.is_cuda else _device_for(echo)
    taps = _as(torch.as_tensor(taps, dtype=torch.float32).reshape(-1), dev, torch.float32)
    e = _as(echo, dev, torch.float32)
    B, N = e.shape
    L = int(taps.numel())
    M = N + 2 * pad - L + 1
    if M <= 0:
        raise RuntimeError("Kernel size can't be greater than actual input size")     # what F.conv1d raises
    with _Scope(dev):
        out = torch.empty((B, M), dtype=torch.float32, device=dev)
        _lib.check(lib.diffus_rows_conv1d(_ptr(e), B, N, _ptr(taps), L, pad, _ptr(out), _stream(dev)), "diffus_rows_conv1d")
    return out.to(echo.device), e, taps


class _PulseFn(torch.autograd.Function):
    """out = rows_conv1d(echo, pulse); backward via diffus_rows_conv1d_bwd (d/d echo: the transposed correlation; d/d pulse:
    fixed-order block partials, bitwise repeatable)."""

    @staticmethod
    def forward(ctx, echo, taps, pad):
        out, e, k = _pulse_launch(echo, taps, pad)
        ctx.save_for_backward(e, k)       # torch raises if either is the caller's tensor and is edited in place
        ctx.pad = pad
        ctx.meta = (echo.device, echo.dtype)
        ctx.tmeta = (taps.device, taps.dtype, tuple(taps.shape)) if isinstance(taps, torch.Tensor) else None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        lib = _lib.load()
        e, k = ctx.saved_tensors
        dev = e.device
        B, N = e.shape
        L = int(k.numel())
        need_e = ctx.needs_input_grad[0]
        need_k = ctx.needs_input_grad[1]
        with _Scope(dev):
            g = _as(gout, dev, torch.float32)
            gin = torch.empty((B, N), dtype=torch.float32, device=dev) if need_e else None
            gk = torch.empty(L, dtype=torch.float32, device=dev) if need_k else None
            nws = lib.diffus_rows_conv1d_bwd_workspace_bytes(B, N, L, ctx.pad) if need_k else 0
            ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
            _lib.check(lib.diffus_rows_conv1d_bwd(_ptr(e), B, N, _ptr(k), L, ctx.pad, _ptr(g), _ptr(gin), _ptr(gk), _ptr(ws),
                                                  nws, _stream(dev)), "diffus_rows_conv1d_bwd")
        out_e = gin.to(device=ctx.meta[0], dtype=ctx.meta[1]) if need_e else None
        out_k = None
        if need_k:
            tdev, tdt, tshape = ctx.tmeta
            out_k = gk.reshape(tshape).to(device=tdev, dtype=tdt)
        return out_e, out_k, None


class UltrasoundRenderer:
    def __init__(self, num_samples: int, attenuation_coeff: float = 0.5):
        """Constructor of reference src/renderer.py:19-25: `num_samples` steps are taken along every ray (one voxel
        apart), and the echo of step k is damped by exp(-attenuation_coeff * k)."""
        self.num_samples = num_samples
        self.attenuation_coeff = attenuation_coeff

    @staticmethod
    def compute_reflection_coeff(Z1: torch.Tensor, Z2: torch.Tensor) -> torch.Tensor:
        """Amplitude reflection coefficient (Z2-Z1)/(Z1+Z2) (reference :27-33).
        Host-side convenience on caller tensors; the hot path computes it in-kernel."""
        return (Z2 - Z1) / (Z1 + Z2)

    @staticmethod
    def trace_ray(volume, source, directions, num_samples: int, start: int, *, sampler="nearest"):
        """reference :90-180 -> (x, y, z, ray_values), each (n_rays, num_samples): the voxel indices of every sample
        point and the impedance there.  `start` is a required argument like in the reference, where it only reaches
        the visualisation (:178 -> :741): it does not change what is returned."""
        out = trace_rays(volume, source, directions, num_samples, sampler, want=("imp", "idx"))
        dev = volume.device
        idx = out["idx"][:, 0].to(dev)
        return idx[0], idx[1], idx[2], out["imp"][0].to(dev)

    def simulate_rays(self, volume, source, directions, num_samples: int = 0, MRI: bool = False, start=0, *,
                      sampler="nearest"):
        """reference :35-71 -> (x, y, z, R) with R (n_rays, num_samples-1) the reflection coefficients between
        consecutive samples -- squeezed to 1-D for a single ray like the reference's `R.squeeze(0)` --, or just the
        impedances Z1 (n_rays, num_samples-1) when MRI.  `start` is passed on to trace_ray (no effect on values)."""
        if num_samples == 0:
            num_samples = self.num_samples
        out = trace_rays(volume, source, directions, num_samples, sampler, want=("imp", "refl", "idx"))
        dev = volume.device
        if MRI:
            return out["imp"][0, :, :-1].to(dev)
        idx = out["idx"][:, 0].to(dev)
        return idx[0], idx[1], idx[2], out["refl"][0].squeeze(0).to(dev)

    def plot_beam_frame(self, volume: torch.Tensor, source: torch.Tensor, directions: torch.Tensor,
                        angle: float = 45.0, plot: bool = True, artifacts: bool = False, ax=None, cmap=None,
                        std_radial: float = 0.01, std_local: float = 0.15, max_sigma: float = 4.0,
                        alpha: float = 5, start: float = 0, *, sampler: str = "nearest",
                        return_indices: bool = True, layout: str = "auto", seed=None, **kwargs):
        """Simulate the fan frame of one pose (reference src/renderer.py:201-275).

        volume (d0,d1,d2) impedance; source (3,); directions (n_rays,3) unit vectors.
        `angle`, `plot`, `ax`, `cmap` are accepted and, as in the reference, never read.
        Returns (x, y, z, processed_output): three (n_rays, num_samples-start) int64
        index planes (None when return_indices=False) and the float32 frame, on
        volume.device.
        """
        if torch.as_tensor(source).numel() != 3:
            raise ValueError("source must have 3 components")
        res = render_poses(volume, source, directions, self.num_samples, self.attenuation_coeff, start=start,
                           sampler=sampler, return_indices=return_indices, layout=layout, _squeeze_pose=True)
        dev = volume.device
        frame = res[0] if return_indices else res
        squeezed = frame.dim() == 2        # the no-grad path hands back (R,N1) / (3,R,N1) buffers: no indexing ops here
        if not squeezed:
            frame = frame[0]
        if artifacts:       # reference :264-273: speckle -> lateral blur -> sharpen (float64 result)
            from .artifacts import apply_artifacts
            frame = apply_artifacts(frame, std_radial=std_radial, std_local=std_local, max_sigma=max_sigma,
                                    alpha=alpha, seed=seed)
        if frame.device != dev:
            frame = frame.to(dev)
        if return_indices:
            idx = res[1]
            if idx.device != dev:
                idx = idx.to(dev)
            if squeezed:
                x, y, z = idx.unbind(0)
                return x, y, z, frame
            return idx[0, 0], idx[1, 0], idx[2, 0], frame
        return None, None, None, frame
