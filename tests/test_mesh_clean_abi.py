"""CPU-side checks of the mesh clean-up entry points (include/mvskit_engine.h: mvs_mesh_pruning, mvs_mesh_smoothing,
mvs_engine_mesh_components, mvs_engine_mesh_prune, mvs_engine_mesh_smooth): every engine library exports them, the structs are 16 bytes
with the header's defaults, and bad arguments are refused in the header's order before the handle is read or a device is touched, with
nothing written through an output pointer."""
import ctypes as C
import os

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_mesh_pruning", "mvs_default_mesh_smoothing", "mvs_engine_mesh_components", "mvs_engine_mesh_prune", "mvs_engine_mesh_smooth")
HEADER = os.path.join(build.ROOT, "include", "mvskit_engine.h")


def test_header_declares_them():
    text = open(HEADER).read()
    for name in SYMBOLS + ("mvs_mesh_pruning", "mvs_mesh_smoothing"):
        assert name + "(" in text or name + ";" in text, name
    # aliasing and the open boundaries are part of the contract
    assert "ALIASES" in text and "NOT PINNED" in text


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    P, S = engine.MeshPruning, engine.MeshSmoothing
    assert C.sizeof(P) == 16 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("min_triangles", 0), ("largest_only", 8), ("pad", 12)]
    assert C.sizeof(S) == 16 and [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("iterations", 0), ("lam", 4), ("mu", 8), ("pad", 12)]
    p = P(-5, -5, -5)
    lib.mvs_default_mesh_pruning(C.byref(p))
    assert (p.min_triangles, p.largest_only) == (1, 0)
    s = S(-5, -5.0, -5.0, -5)
    lib.mvs_default_mesh_smoothing(C.byref(s))
    assert s.iterations == 10 and s.lam == np.float32(0.5) and s.mu == np.float32(-0.53)
    lib.mvs_default_mesh_pruning(None)  # ignored
    lib.mvs_default_mesh_smoothing(None)

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    out_v = np.full((8, 3), -7, np.float32)
    out_t = np.full((8, 3), -7, np.int32)
    label, ntris, vmap = (np.full(8, -7, np.int32) for _ in range(3))
    nc, nvo, nto = (C.c_int64(-7) for _ in range(3))
    vtp, trp, ovp, otp, lbp, ntp, vmp = (a.ctypes.data_as(vp) for a in (verts, tris, out_v, out_t, label, ntris, vmap))
    big = (1 << 30) + 1
    bad_counts = ((-1, 8), (8, -1), (big, 8), (8, big))

    # mvs_engine_mesh_components: the counts, tris, the engine
    f = lib.mvs_engine_mesh_components
    for nv, nt in bad_counts:
        assert f(None, nv, nt, None, lbp, ntp, C.byref(nc)) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert f(None, 8, 8, None, lbp, ntp, C.byref(nc)) == MVS_ERR_ARG and err(b"tris null")
    assert f(None, 8, 8, trp, lbp, ntp, C.byref(nc)) == MVS_ERR_ARG and err(b"no engine")
    assert f(None, 8, 0, None, None, None, None) == MVS_ERR_ARG and err(b"no engine")  # every output may be null
    assert f(None, 0, 0, None, None, None, C.byref(nc)) == MVS_ERR_ARG and err(b"no engine")
    assert f(None, 1 << 30, 1 << 30, trp, lbp, ntp, C.byref(nc)) == MVS_ERR_ARG and err(b"no engine")  # the limit itself is allowed

    # mvs_engine_mesh_prune: p, min_triangles, largest_only, the counts, verts, tris, the size pointers, the caps, the engine -- each with
    # every later argument bad too
    def pr(min_triangles=1, largest_only=0):
        return C.byref(P(min_triangles, largest_only, 0))

    g = lib.mvs_engine_mesh_prune
    assert g(None, None, -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"pruning null")
    for m in (0, -3):
        assert g(None, pr(m, 2), -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"min_triangles"), m
    for lo in (2, -1):
        assert g(None, pr(1, lo), -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"largest_only"), lo
    for nv, nt in bad_counts:
        assert g(None, pr(), nv, None, nt, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert g(None, pr(), 8, None, 8, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert g(None, pr(), 8, vtp, 8, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert g(None, pr(), 8, vtp, 8, trp, -1, ovp, -1, otp, vmp, None, C.byref(nto)) == MVS_ERR_ARG and err(b"null")
    assert g(None, pr(), 8, vtp, 8, trp, -1, ovp, -1, otp, vmp, C.byref(nvo), None) == MVS_ERR_ARG and err(b"null")
    assert g(None, pr(), 8, vtp, 8, trp, -1, ovp, 8, otp, vmp, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, pr(), 8, vtp, 8, trp, 8, ovp, -1, otp, vmp, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, pr(), 8, vtp, 8, trp, 8, ovp, 8, otp, vmp, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, pr(1 << 40, 1), 0, None, 0, None, 0, None, 0, None, None, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_mesh_smooth: s, iterations, lambda, mu, the counts, the pointers, the engine
    def sm(iterations=10, lam=0.5, mu=-0.53):
        return C.byref(S(iterations, lam, mu, 0))

    h = lib.mvs_engine_mesh_smooth
    nan, inf = float("nan"), float("inf")
    assert h(None, None, -1, None, -1, None, None) == MVS_ERR_ARG and err(b"smoothing null")
    for it in (-1, 1001):
        assert h(None, sm(it, nan, nan), -1, None, -1, None, None) == MVS_ERR_ARG and err(b"iterations"), it
    for x in (0.0, 1.0, -0.5, 1.5, nan, inf):
        assert h(None, sm(lam=x, mu=nan), -1, None, -1, None, None) == MVS_ERR_ARG and err(b"lambda"), x
    for x in (-1.0, 0.25, -2.0, nan, -inf):
        assert h(None, sm(mu=x), -1, None, -1, None, None) == MVS_ERR_ARG and err(b"mu "), x
    for nv, nt in bad_counts:
        assert h(None, sm(), nv, None, nt, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert h(None, sm(), 8, None, 8, trp, ovp) == MVS_ERR_ARG and err(b"null")
    assert h(None, sm(), 8, vtp, 8, None, ovp) == MVS_ERR_ARG and err(b"null")
    assert h(None, sm(), 8, vtp, 8, trp, None) == MVS_ERR_ARG and err(b"null")
    assert h(None, sm(), 8, vtp, 8, trp, ovp) == MVS_ERR_ARG and err(b"no engine")
    assert h(None, sm(0, 0.999, 0.0), 0, None, 0, None, None) == MVS_ERR_ARG and err(b"no engine")  # the ends of the ranges that are allowed
    assert h(None, sm(1000, 1e-6, -0.999), 8, vtp, 0, None, ovp) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    for a in (verts, tris, out_v, out_t, label, ntris, vmap):
        assert (a == -7).all()
    assert (nc.value, nvo.value, nto.value) == (-7, -7, -7)
