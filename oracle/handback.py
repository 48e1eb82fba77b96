"""The sparse gradient hand-back, restated in numpy.

TEST INFRASTRUCTURE ONLY (oracle).  What diffus_gradbuf_flush (diffus_amd/csrc/layout.hip: gradbuf_flush_kernel,
gradbuf_flush_dense_kernel) does to the bricked gradient scratch, its touched-brick flags and the canonical tensor, so
that multi-rank logic (diffus_amd.distributed.allreduce_touched) can be tested end to end without a GPU.

Brick geometry (diffus_device.hpp: vox_off, diffus_host.hpp: bricked_floats): 4 x 4 x 2 voxels per brick,
nb = (ceil(d0/4), ceil(d1/4), ceil(d2/2)), brick (bx*nb1 + by)*nb2 + bz, in-brick offset ((x&3)<<3)|((y&3)<<1)|(z&1),
32 floats per brick; the slots of an edge brick that fall outside the volume exist in the scratch but not in `out`.

Flags: 0 nothing; 1 live (the scatter added into the scratch this step); 2 stale (left by a PERSISTENT flush: `out`
holds the previous step's values there and the scratch is zero).
"""
from __future__ import annotations

import numpy as np

STORE, ACCUMULATE, PERSISTENT, DENSE = 0, 1, 2, 3        # include/diffus_hip.h DIFFUS_FLUSH_*
BRICK_FLOATS = 32


def brick_grid(shape):
    d0, d1, d2 = (int(x) for x in shape)
    return (d0 + 3) // 4, (d1 + 3) // 4, (d2 + 1) // 2


def brick_count(shape) -> int:
    nb0, nb1, nb2 = brick_grid(shape)
    return nb0 * nb1 * nb2


def brick(dense: np.ndarray) -> np.ndarray:
    """Canonical (d0,d1,d2) -> bricked (n_bricks * 32,), the slots outside the volume zero (False for a bool volume)."""
    d0, d1, d2 = dense.shape
    nb0, nb1, nb2 = brick_grid(dense.shape)
    pad = np.zeros((4 * nb0, 4 * nb1, 2 * nb2), dtype=dense.dtype)
    pad[:d0, :d1, :d2] = dense
    return np.ascontiguousarray(pad.reshape(nb0, 4, nb1, 4, nb2, 2).transpose(0, 2, 4, 1, 3, 5)).reshape(-1)


def unbrick(bricked: np.ndarray, shape) -> np.ndarray:
    """Bricked (n_bricks * 32,) -> canonical (d0,d1,d2); the slots outside the volume are dropped."""
    d0, d1, d2 = (int(x) for x in shape)
    nb0, nb1, nb2 = brick_grid(shape)
    full = np.asarray(bricked).reshape(nb0, nb1, nb2, 4, 4, 2).transpose(0, 3, 1, 4, 2, 5).reshape(4 * nb0, 4 * nb1, 2 * nb2)
    return np.ascontiguousarray(full[:d0, :d1, :d2])


def flush(bricked: np.ndarray, touched: np.ndarray, out: np.ndarray, mode: int) -> None:
    """diffus_gradbuf_flush(bricked, touched, *out.shape, out, mode), in place on the three arrays.

    bricked: float32 (n_bricks * 32,); touched: int32 (n_bricks,); out: float32 (d0,d1,d2), any strides.
    STORE / ACCUMULATE / PERSISTENT visit the bricks with a flag != 0: a stale one (2) contributes zeros (its scratch
    is neither read nor cleared), any other one its scratch, which is then zeroed; the brick's voxels of `out` are
    overwritten (STORE, PERSISTENT) or added into in float32 (ACCUMULATE); the flag becomes 2 if the mode is PERSISTENT
    and it was 1, else 0.  DENSE writes every voxel of `out`: the scratch of the bricks flagged 1 (then zeroed), zeros
    everywhere else; every flag becomes 0."""
    if mode not in (STORE, ACCUMULATE, PERSISTENT, DENSE):
        raise ValueError(f"unknown flush mode {mode}")
    nb = brick_count(out.shape)
    assert bricked.dtype == np.float32 and bricked.size == nb * BRICK_FLOATS, (bricked.dtype, bricked.size, nb)
    assert touched.dtype == np.int32 and touched.size == nb and out.dtype == np.float32
    b = bricked.reshape(nb, BRICK_FLOATS)
    f = touched.copy()
    live = (f == 1) if mode == DENSE else ((f != 0) & (f != 2))
    vals = np.zeros((nb, BRICK_FLOATS), dtype=np.float32)
    vals[live] = b[live]
    b[live] = 0.0
    v = unbrick(vals, out.shape)
    if mode == DENSE:
        touched[f != 0] = 0
        out[...] = v
        return
    sel = f != 0
    touched[sel] = np.where((f[sel] == 1) & (mode == PERSISTENT), 2, 0).astype(np.int32)
    covered = unbrick(np.repeat(sel, BRICK_FLOATS), out.shape)
    if mode == ACCUMULATE:
        out[covered] = out[covered] + v[covered]
    else:
        out[covered] = v[covered]
