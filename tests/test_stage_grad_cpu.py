"""CPU-side checks of the stage backward entry points (diffus_sample_points_bwd, diffus_trace_rays_bwd,
diffus_rows_conv1d_bwd): declared, exported, and validating their arguments before anything reaches HIP.
No kernel is launched here."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("diffus_sample_points_bwd", "diffus_trace_rays_bwd", "diffus_trace_rays_bwd_workspace_bytes",
       "diffus_rows_conv1d_bwd", "diffus_rows_conv1d_bwd_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from diffus_amd import build, _lib
    build.build()
    return _lib.load()


def test_new_entry_points_are_declared_exported_and_cite_the_reference(lib):
    from diffus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "diffus_hip.h")).read()
    for fn in NEW:
        assert fn in _lib.EXPORTS
        assert getattr(lib, fn) is not None
    for fn in ("diffus_sample_points_bwd", "diffus_trace_rays_bwd", "diffus_rows_conv1d_bwd"):
        i = txt.index("int " + fn + "(")
        comment = txt[txt.rfind("/*", 0, i): i]
        assert "src/renderer.py:" in comment, fn
    assert lib.diffus_abi_version() == 8


def test_workspace_arithmetic(lib):
    assert lib.diffus_trace_rays_bwd_workspace_bytes(1, 1) == 256
    assert lib.diffus_trace_rays_bwd_workspace_bytes(32, 256) == 32 * 256 * 3 * 4
    assert lib.diffus_trace_rays_bwd_workspace_bytes(0, 4) == 0
    assert lib.diffus_trace_rays_bwd_workspace_bytes(4, -1) == 0
    # one float64 partial per (block, tap); blocks = min(ceil(B*M / 256), 256), M = N + 2 pad - L + 1
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(1, 10, 3, 1) == 256                      # M = 10: 1 block x 3 taps
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(4, 121, 10, 5) == 2 * 10 * 8 + 96        # M = 122: 2 blocks, aligned
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(1000, 1000, 7, 3) == 256 * 7 * 8         # capped at 256 blocks
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(1, 3, 10, 0) == 0                        # M <= 0
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(0, 10, 3, 1) == 0
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(1, 10, 0, 1) == 0
    assert lib.diffus_rows_conv1d_bwd_workspace_bytes(1, 10, 3, -1) == 0


def test_sample_points_bwd_validation(lib):
    f = (C.c_float * 64)()
    p = C.cast(f, C.c_void_p)

    def call(vol=p, d=(2, 2, 2), layout=0, pts=p, n=4, sampler=0, gv=p, gvol=p, gp=p):
        return lib.diffus_sample_points_bwd(vol, *d, layout, pts, n, sampler, gv, gvol, gp, None)

    assert call(vol=None) == -1
    assert call(pts=None) == -1
    assert call(gv=None) == -1
    assert call(n=0) == -1
    assert call(n=-3) == -1
    assert call(d=(0, 2, 2)) == -1
    assert call(d=(2, -1, 2)) == -1
    assert call(sampler=2) == -1
    assert call(layout=3) == -1
    assert call(d=(1 << 25, 2, 2)) == -2
    assert call(gvol=None, gp=None) == 0          # nothing asked for: nothing launched


def test_trace_rays_bwd_validation(lib):
    f = (C.c_float * 64)()
    p = C.cast(f, C.c_void_p)
    ok = dict(vol=p, d=(2, 2, 2), layout=0, src=p, sdt=0, dirs=p, ddt=0, P=1, R=1, S=4, sampler=1, gimp=p, grefl=p,
              gvol=p, gsrc=p, gdirs=p, ws=p, nws=256)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.diffus_trace_rays_bwd(a["vol"], *a["d"], a["layout"], a["src"], a["sdt"], a["dirs"], a["ddt"], a["P"],
                                         a["R"], a["S"], a["sampler"], a["gimp"], a["grefl"], a["gvol"], a["gsrc"],
                                         a["gdirs"], a["ws"], a["nws"], None)

    assert call(vol=None) == -1
    assert call(src=None) == -1
    assert call(dirs=None) == -1
    assert call(P=0) == -1
    assert call(R=-1) == -1
    assert call(S=0) == -1
    assert call(d=(2, 0, 2)) == -1
    assert call(sampler=5) == -1
    assert call(layout=7) == -1
    assert call(sdt=2) == -1
    assert call(d=(2, 2, 1 << 25)) == -2
    assert call(ws=None) == -4                    # trilinear d/d source needs the per-ray partials
    assert call(nws=255) == -4
    # no incoming gradient and nothing that needs a launch: returns before touching the device
    assert call(gimp=None, grefl=None, gsrc=None, gdirs=None) == 0
    assert call(sampler=0, gsrc=None, gdirs=None, ws=None, nws=0, gimp=None, grefl=None) == 0


def test_rows_conv1d_bwd_validation(lib):
    f = (C.c_float * 256)()
    p = C.cast(f, C.c_void_p)

    def call(inp=p, B=2, N=10, k=p, L=3, pad=1, gout=p, gin=p, gk=p, ws=p, nws=1024):
        return lib.diffus_rows_conv1d_bwd(inp, B, N, k, L, pad, gout, gin, gk, ws, nws, None)

    assert call(inp=None) == -1
    assert call(k=None) == -1
    assert call(gout=None) == -1
    assert call(B=0) == -1
    assert call(N=0) == -1
    assert call(L=0) == -1
    assert call(pad=-1) == -1
    assert call(N=2, L=5, pad=0) == -1           # kernel longer than the padded row
    assert call(ws=None) == -4
    assert call(nws=100) == -4
    assert call(gin=None, gk=None, ws=None, nws=0) == 0
