#!/usr/bin/env python3
"""One-pass step time (CapturedStep: forward, loss, backward, gradient hand-back, one captured graph) of a sector fan
against array probes with one origin per ray (DIFFUS_SRC_PER_RAY), at the config-3 shape: 32 poses x 256 rays x 512
steps, 256^3 phantom, trilinear.  Device events around 200 replays after 20 warm-up replays; prints one JSON object.
    tools/time_array_probe.py [--steps 200] [--out FILE] [--only fan,linear,tilted,convex]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffus_amd as da  # noqa: E402
from diffus_amd.phantom import phantom, pose_ring  # noqa: E402

N, P, R, S = 256, 32, 256, 512


def probes(kind):
    """-> sources (P,3) or (P,R,3), directions (P,R,3), float32 on the GPU; the array poses sit on the fan ring."""
    src, dirs = pose_ring(N, P, R)
    if kind == "fan":
        return torch.from_numpy(src).cuda(), torch.from_numpy(dirs).cuda()
    S_, D_ = [], []
    for p in range(P):
        look = dirs[p, R // 2].astype(np.float64)
        look[2] = 0.0
        look /= np.linalg.norm(look)
        side = np.array([-look[1], look[0], 0.0])
        c = torch.from_numpy(src[p].astype(np.float64))
        if kind == "linear":
            s, d = da.linear_array(c, look, side, R, 0.25 * N)
        elif kind == "tilted":
            s, d = da.linear_array(c, look + np.array([0.0, 0.0, 0.15]), side + np.array([0.0, 0.0, 0.3]), R, 0.25 * N)
        else:
            s, d = da.convex_array(c - 0.1 * N * torch.from_numpy(look), look, side, 0.1 * N, np.deg2rad(60.0), R)
        S_.append(s.float())
        D_.append(d.float())
    return torch.stack(S_).contiguous().cuda(), torch.stack(D_).contiguous().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="fan,linear,tilted,convex")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_array_probe.py needs a GPU")
    vol = torch.from_numpy(phantom(N)).cuda()
    res = {"shape": {"P": P, "R": R, "S": S, "n": N, "sampler": "trilinear"}, "steps": a.steps, "ms_per_step": {}}
    for kind in a.only.split(","):
        s, d = probes(kind)
        st = da.CapturedStep(vol, s, d, S, 1e-4, "trilinear")
        st.capture()
        for _ in range(a.warmup):
            st.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            st.replay()
        e1.record()
        torch.cuda.synchronize()
        res["ms_per_step"][kind] = e0.elapsed_time(e1) / a.steps
        res.setdefault("fans_planar", {})[kind] = st.fans_planar
        del st
    if "fan" in res["ms_per_step"]:
        res["ratio_to_fan"] = {k: v / res["ms_per_step"]["fan"] for k, v in res["ms_per_step"].items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
