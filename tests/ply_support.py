"""PLY files of the tests (a helper module like oracle_binding.py): the numpy restatement of the file mvs_engine_export_ply and the
host mirror's PatchManager::writePly write, with its inputs at a level, and the writer and camera of the small data set that
tests/test_seed_plys.py and tests/test_gpu_seed_patches.py read seeds from."""
import math
import os
import struct

import numpy as np

from mvskit_amd import engine

F = np.float32
GOLDEN_JPG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg", "baseline_444.jpg")  # 40 x 30
W, H, NV = 40, 30, 4


def restate_ply(recs, P_level, pyr, binary=False):
    """The PLY file of `recs` (mvs_patch records in pool order). P_level[v]: the level's 3x4 projection (float32); pyr[v]: the level's
    H x W x 3 uint8 image."""
    n = recs.shape[0]
    nv = len(pyr)
    X = recs["coord"].astype(F)
    col = np.zeros((n, 3), F)
    denom = np.zeros(n, np.int64)
    nim = recs["nimages"]
    for k in range(int(nim.max()) if n else 0):
        img = recs["images"][:, k].astype(np.int64)
        listed = (k < nim) & (img < nv)
        denom += listed
        for v in range(nv):
            sel = listed & (img == v)
            if not sel.any():
                continue
            q = P_level[v].astype(F).ravel()
            Xs = X[sel]
            z = q[8] * Xs[:, 0] + q[9] * Xs[:, 1] + q[10] * Xs[:, 2] + q[11] * Xs[:, 3]
            with np.errstate(divide="ignore", invalid="ignore"):
                x = (q[0] * Xs[:, 0] + q[1] * Xs[:, 1] + q[2] * Xs[:, 2] + q[3] * Xs[:, 3]) / z
                y = (q[4] * Xs[:, 0] + q[5] * Xs[:, 1] + q[6] * Xs[:, 2] + q[7] * Xs[:, 3]) / z
            H, W = pyr[v].shape[:2]
            ok = (z > 0) & (x >= 0) & (y >= 0) & (x < F(W - 1)) & (y < F(H - 1))
            x, y = x[ok], y[ok]
            lx, ly = x.astype(np.int64), y.astype(np.int64)
            dx1 = x - lx.astype(F)
            dx0 = F(1) - dx1
            dy1 = y - ly.astype(F)
            dy0 = F(1) - dy1
            f00, f01, f10, f11 = dx0 * dy0, dx0 * dy1, dx1 * dy0, dx1 * dy1
            im = pyr[v].astype(F)
            term = (im[ly, lx] * f00[:, None] + im[ly + 1, lx] * f01[:, None]) + (im[ly, lx + 1] * f10[:, None] + im[ly + 1, lx + 1] * f11[:, None])
            rows = np.nonzero(sel)[0][ok]
            col[rows] = col[rows] + term.astype(F)
    rgb = np.full((n, 3), 128, np.int64)
    has = denom > 0
    rgb[has] = np.minimum(255, np.floor(col[has] / denom[has, None].astype(F) + F(0.5)).astype(np.int64))
    head = (f"ply\nformat {'binary_little_endian' if binary else 'ascii'} 1.0\nelement vertex {n}\nproperty float x\nproperty float y\n"
            "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar diffuse_red\nproperty uchar diffuse_green\n"
            "property uchar diffuse_blue\nend_header\n").encode()
    if binary:
        body = np.zeros(n, engine.PLY_VERTEX_DTYPE)
        body["xyz"] = recs["coord"][:, :3]
        body["normal"] = recs["normal"][:, :3]
        body["rgb"] = rgb
        return head + body.tobytes()
    lines = []
    for i in range(n):
        c, nm = recs["coord"][i], recs["normal"][i]
        lines.append("%g %g %g %g %g %g %d %d %d\n" % (c[0], c[1], c[2], nm[0], nm[1], nm[2], rgb[i, 0], rgb[i, 1], rgb[i, 2]))
    return head + "".join(lines).encode()


def level_inputs(e, sc, level, sizes=None):
    """sizes: the per-view (width, height) given to Engine.set_scene (top-left crops), default every view at sc.W x sc.H"""
    P = []
    for v in range(sc.nviews):
        p = np.asarray(sc.P[v], F).ravel().copy()
        for _ in range(level):
            p[:8] = p[:8] / F(2)
        P.append(p)
    wh = [(sc.W, sc.H)] * sc.nviews if sizes is None else sizes
    pyr = [np.asarray(sc.images[v], np.uint8)[:wh[v][1], :wh[v][0]] if level == 0 else e.pyramid(v, level) for v in range(sc.nviews)]
    return P, pyr


def parse_ascii(data):
    end = data.index(b"end_header\n") + len(b"end_header\n")
    rows = [r.split() for r in data[end:].decode().split("\n") if r]
    return rows


def write_ply(path, fmt, xyz, normals=None, extra_colour=False, faces=None):
    n = len(xyz)
    head = ["ply", f"format {fmt} 1.0", "comment written by tests/test_seed_plys.py", f"element vertex {n}",
            "property float x", "property float y", "property double z" if fmt != "ascii" else "property float z"]
    if extra_colour:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    if faces is not None:
        head += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        e = "<" if fmt == "binary_little_endian" else ">"
        for i in range(n):
            if fmt == "ascii":
                vals = [repr(float(v)) for v in xyz[i]]
                if extra_colour:
                    vals += ["10", "20", "30"]
                if normals is not None:
                    vals += [repr(float(v)) for v in normals[i]]
                f.write((" ".join(vals) + "\n").encode())
            else:
                f.write(struct.pack(e + "ffd", *[float(v) for v in xyz[i]]))
                if extra_colour:
                    f.write(bytes([10, 20, 30]))
                if normals is not None:
                    f.write(struct.pack(e + "fff", *[float(v) for v in normals[i]]))
        for face in faces or []:
            if fmt == "ascii":
                f.write((f"{len(face)} " + " ".join(str(v) for v in face) + "\n").encode())
            else:
                f.write(struct.pack(e + "B" + "i" * len(face), len(face), *face))


def euler_camera(a, b, g, t, fx=60.0, fy=60.0, cx=W / 2.0, cy=H / 2.0, skew=0.0):
    """CONTOUR2 line of a camera (camera.cpp:117-134: K = [[fx, skew, cx], [0, fy, cy], [0, 0, 1]]; quat2proj 241-261) and its rotation."""
    s1, s2, s3, c1, c2, c3 = (math.sin(math.radians(a)), math.sin(math.radians(b)), math.sin(math.radians(g)),
                              math.cos(math.radians(a)), math.cos(math.radians(b)), math.cos(math.radians(g)))
    R = np.array([[c2 * c3, c3 * s2 * s1 - s3 * c1, c3 * s2 * c1 + s3 * s1], [s3 * c2, s3 * s2 * s1 + c3 * c1, s3 * s2 * c1 - c3 * s1],
                  [-s2, c2 * s1, c2 * c1]])
    text = "CONTOUR2\n%r %r %s %r %r 0\n%r %r %r\n%r %r %r\n" % ((float(fx), float(fy), "0" if skew == 0 else repr(float(skew)))
                                                            + tuple(float(v) for v in (cx, cy, a, b, g, t[0], t[1], t[2])))
    return text, R
