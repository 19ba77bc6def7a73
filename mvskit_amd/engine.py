"""ctypes binding of the C ABI in include/mvskit_engine.h, include/mvskit_texture.h and include/mvskit_seams.h.

There is no CPU path: if the HIP library is missing or no GPU is visible, creating an Engine raises."""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
import zlib

import numpy as np

from . import synth
from .abi import *  # noqa: F401,F403  (abi.__all__: the constants, dtypes, structs, SIGNATURES, EngineError and load_library)
from .synth import MAX_IMAGES, PATCH_DTYPE  # noqa: F401  (PATCH_DTYPE mirrors mvs_patch at 32 list slots)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _verts(a):
    """[n, 3] float32, C order: mesh vertices, and the world points of the seed calls"""
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


_points = _verts


def _tris(a):
    """[m, 3] int32, C order"""
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3)


def _record(s):
    """a struct of numbers as a dictionary: int for the integer fields, float for the float fields"""
    return {n: getattr(s, n) for n, _ in s._fields_}


class Engine:
    """One PmMvps instance whose Propagate::run lives on an MI355X (pmmvps/pmmvps.cpp:76-114)."""

    def __init__(self, nviews, list_cap=None, **kw):
        """list_cap: 16, 32 or 64 views per m_images / m_vimages list (which library); default: the smallest that holds `nviews`,
        so that no list is ever cut short.  `dtype` is the record this library takes and returns (192 bytes at 64)."""
        if list_cap is None:
            list_cap = 16 if nviews <= 16 else (32 if nviews <= 32 else 64)
        self.L = load_library(cap=list_cap)
        self.list_cap = self.L.mvs_list_cap()
        self.dtype = synth.patch_dtype((self.L.mvs_patch_bytes() - 64) // 2)
        self.cfg = Config()
        self.L.mvs_default_config(C.byref(self.cfg))
        self.cfg.nviews = nviews
        for k, v in kw.items():
            if not hasattr(self.cfg, k):
                raise AttributeError(k)
            setattr(self.cfg, k, v)
        self.h = C.c_void_p()
        self._check(self.L.mvs_engine_create(C.byref(self.cfg), C.byref(self.h)))

    def _check(self, status):
        if status != 0:
            raise EngineError(f"mvskit engine error {status}: {self.L.mvs_last_error().decode()}", status)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.mvs_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- views
    def set_scene(self, scene, masks=None, sizes=None):
        """sizes: one (width, height) per view -- the view is the top-left crop of the scene's image (and mask) to that size, which
        leaves its projection valid; default: every view at scene.W x scene.H."""
        n = scene.nviews
        descs = (ViewDesc * n)()
        keep = []
        for v in range(n):
            w, h = (scene.W, scene.H) if sizes is None else sizes[v]
            img = np.ascontiguousarray(np.asarray(scene.images[v], dtype=np.uint8)[:h, :w])
            keep.append(img)
            descs[v].width, descs[v].height = w, h
            P = np.ascontiguousarray(scene.P[v], dtype=np.float32).ravel()
            for k in range(12):
                descs[v].P[k] = float(P[k])
            descs[v].rgb = img.ctypes.data
            descs[v].mask = None
            if masks is not None and masks[v] is not None:  # masks[v] None: that view has no mask
                m = np.ascontiguousarray(np.asarray(masks[v], dtype=np.uint8)[:h, :w])
                keep.append(m)
                descs[v].mask = m.ctypes.data
        self._check(self.L.mvs_engine_set_views(self.h, n, descs))
        self._view_shapes = [(scene.H, scene.W)] * n if sizes is None else [(h, w) for w, h in sizes]

    def grid_dims(self, v):
        gw, gh = C.c_int(), C.c_int()
        self._check(self.L.mvs_engine_grid_dims(self.h, v, C.byref(gw), C.byref(gh)))
        return gw.value, gh.value

    def pyramid(self, v, level):
        w, h = C.c_int(), C.c_int()
        self._check(self.L.mvs_engine_get_pyramid(self.h, v, level, None, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 3), dtype=np.uint8)
        self._check(self.L.mvs_engine_get_pyramid(self.h, v, level, _ptr(out), C.byref(w), C.byref(h)))
        return out

    def set_refiner(self, mode="halving", max_evals=500, xtol=1e-4):
        """Optim::refinePatch's refiner for the passes and probes that follow: "halving" (the default search) or "converged"
        (Nelder-Mead until xtol or max_evals evaluations; include/mvskit_engine.h, mvs_refiner)."""
        modes = {"halving": REFINE_HALVING, "converged": REFINE_CONVERGED}
        if mode not in modes:
            raise ValueError(f"refiner mode {mode!r}: 'halving' or 'converged'")
        r = Refiner(modes[mode], int(max_evals), float(xtol))
        self._check(self.L.mvs_engine_set_refiner(self.h, C.byref(r)))

    def set_thresholds(self, ncc, before, depth):
        self._check(self.L.mvs_engine_set_thresholds(self.h, ncc, before, depth))

    def thresholds(self):
        a, b, d = C.c_float(), C.c_float(), C.c_int()
        self._check(self.L.mvs_engine_get_thresholds(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return a.value, b.value, d.value

    def update_threshold(self):
        self._check(self.L.mvs_engine_update_threshold(self.h))

    # ---- patches
    def upload_patches(self, recs):
        recs = synth.convert_records(recs, self.dtype)
        self._check(self.L.mvs_engine_upload_patches(self.h, recs.shape[0], _ptr(recs)))

    add_patches = upload_patches

    def seed_patches(self, points, normal_maps, masks=None):
        """DepthNormInit::createPatches' PLY branch on the device (include/mvskit_engine.h, mvs_engine_seed_patches): appends the seed
        patches of `points` (N x 3 world coordinates) to the pool, in point order, and returns how many.  normal_maps[v]: H x W x 3
        float32 in world axes, zero where the view has no normal, or None; masks[v]: H x W uint8 level-0 mask (> 127 = foreground) or
        None.  A view without a mask takes no part (the reference's rule), so masks=None seeds nothing."""
        n = self.cfg.nviews
        if len(normal_maps) != n or (masks is not None and len(masks) != n):
            raise ValueError(f"seed_patches: {n} views, one normal map (and mask) each")
        pts = _points(points)
        shapes = getattr(self, "_view_shapes", None)
        views = (SeedView * n)()
        keep = []  # the maps and masks, until the call has returned
        for v in range(n):
            views[v].normals = views[v].mask = None
            shape = shapes[v] if shapes is not None else None
            if normal_maps[v] is not None:
                m = np.ascontiguousarray(normal_maps[v], dtype=np.float32)
                if shape is not None and m.shape != shape + (3,):
                    raise ValueError(f"seed_patches: normal map {v} has shape {m.shape}, the view is {shape + (3,)}")
                keep.append(m)
                views[v].normals = m.ctypes.data
            if masks is not None and masks[v] is not None:
                k = np.ascontiguousarray(masks[v], dtype=np.uint8)
                if shape is not None and k.shape != shape:
                    raise ValueError(f"seed_patches: mask {v} has shape {k.shape}, the view is {shape}")
                keep.append(k)
                views[v].mask = k.ctypes.data
        added = C.c_int64()
        self._check(self.L.mvs_engine_seed_patches(self.h, pts.shape[0], _ptr(pts), views, C.byref(added)))
        return added.value

    def _seed_random_args(self, depth_min, depth_max, hypotheses, seed, max_tilt, min_ncc):
        """mvs_seed_random from Python values; a scalar range serves every view.  Returns the struct and the arrays it points at."""
        n = self.cfg.nviews
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(depth_min, dtype=np.float32), (n,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(depth_max, dtype=np.float32), (n,)))
        s = SeedRandom(int(hypotheses), int(seed), float(max_tilt), -1.0 if min_ncc is None else float(min_ncc), lo.ctypes.data, hi.ctypes.data)
        return s, (lo, hi)

    def seed_random(self, depth_min, depth_max, hypotheses=8, seed=1, max_tilt=math.pi / 3, min_ncc=None):
        """The cold start (include/mvskit_engine.h, mvs_engine_seed_random): per cell of every view `hypotheses` random planes inside
        [depth_min, depth_max] along the view's optical axis and within max_tilt of the direction to the camera, the best-scoring one
        refined and post-processed on the device; the patches that pass are appended to the pool in (view, cell) order.  Ranges:
        one value per view or a scalar for all.  min_ncc None: the engine's nccThresholdBefore.  Returns how many were appended."""
        s, _ranges = self._seed_random_args(depth_min, depth_max, hypotheses, seed, max_tilt, min_ncc)
        added = C.c_int64()
        self._check(self.L.mvs_engine_seed_random(self.h, C.byref(s), C.byref(added)))
        return added.value

    def seed_random_hypotheses(self, view, cells, depth_min, depth_max, hypotheses=8, seed=1, max_tilt=math.pi / 3, min_ncc=None):
        """The hypotheses seed_random scores, as records: `hypotheses` per listed cell (cy * gw + cx) of `view`, hypothesis k of cells[i]
        at [i * hypotheses + k].  Reads engine state only."""
        s, _ranges = self._seed_random_args(depth_min, depth_max, hypotheses, seed, max_tilt, min_ncc)
        cells = np.ascontiguousarray(cells, dtype=np.int32).ravel()
        out = np.zeros(cells.shape[0] * max(int(hypotheses), 0), dtype=self.dtype)
        self._check(self.L.mvs_engine_seed_random_hypotheses(self.h, C.byref(s), int(view), cells.shape[0], _ptr(cells), _ptr(out)))
        return out

    def seed_points(self, points, hypotheses=4, min_ncc=None):
        """The warm start (include/mvskit_engine.h, mvs_engine_seed_points): per point of `points` (N x 3 world coordinates, the sparse
        points of structure-from-motion) at most `hypotheses` reference views, nearest first, each with the normal turned towards its
        camera; the best-scoring one refined and post-processed on the device; the patches that pass are appended to the pool in point
        order.  min_ncc None: the engine's nccThresholdBefore.  Returns how many were appended."""
        pts = _points(points)
        s = SeedPoints(int(hypotheses), -1.0 if min_ncc is None else float(min_ncc))
        added = C.c_int64()
        self._check(self.L.mvs_engine_seed_points(self.h, C.byref(s), pts.shape[0], _ptr(pts), C.byref(added)))
        return added.value

    def seed_points_hypotheses(self, points, hypotheses=4, min_ncc=None):
        """The hypotheses seed_points scores -> (records, count): count[i] hypotheses of point i at records[i * hypotheses ...], zero
        records in the slots behind.  Reads engine state only."""
        pts = _points(points)
        s = SeedPoints(int(hypotheses), -1.0 if min_ncc is None else float(min_ncc))
        out = np.zeros(pts.shape[0] * max(int(hypotheses), 0), dtype=self.dtype)
        count = np.zeros(pts.shape[0], np.int32)
        self._check(self.L.mvs_engine_seed_points_hypotheses(self.h, C.byref(s), pts.shape[0], _ptr(pts), _ptr(out), _ptr(count)))
        return out, count

    def depth_ranges(self, points, margin=0.1):
        """Per view the depth range of the points that pass its gate, widened by `margin` -> (depth_min, depth_max, count): float32
        arrays that seed_random takes as they are, and the number of qualifying points per view (a view with none: 0, 0)."""
        pts = _points(points)
        n = self.cfg.nviews
        lo, hi, count = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64)
        self._check(self.L.mvs_engine_depth_ranges(self.h, pts.shape[0], _ptr(pts), float(margin), _ptr(lo), _ptr(hi), _ptr(count)))
        return lo, hi, count

    def reserve(self, list_entries=0):
        """Sizes the cell indexes up front (0: MAX_NUM_OF_PATCHES per cell of every view): no allocation inside the iterations."""
        self._check(self.L.mvs_engine_reserve(self.h, int(list_entries)))

    def clear_patches(self):
        self._check(self.L.mvs_engine_clear_patches(self.h))

    def num_patches(self):
        n = C.c_int64()
        self._check(self.L.mvs_engine_num_patches(self.h, C.byref(n)))
        return n.value

    def patches(self):
        n = C.c_int64()
        self._check(self.L.mvs_engine_download_patches(self.h, 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=self.dtype)
        if n.value:
            self._check(self.L.mvs_engine_download_patches(self.h, n.value, _ptr(out), C.byref(n)))
        return out

    def export_ply(self, binary=False):
        """PatchManager::writePly of the alive pool as the bytes of a PLY file: ASCII (what std::ostream wrote) or, with binary=True,
        binary_little_endian with the same numbers (include/mvskit_engine.h, mvs_engine_export_ply)."""
        fmt = PLY_BINARY_LE if binary else PLY_ASCII
        n = C.c_int64()
        self._check(self.L.mvs_engine_export_ply(self.h, fmt, 0, None, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        self._check(self.L.mvs_engine_export_ply(self.h, fmt, n.value, buf, C.byref(n)))
        return buf.raw[:n.value]

    def points(self):
        """The alive pool as PLY vertices: a structured array with xyz (f4 x 3), normal (f4 x 3) and rgb (u1 x 3), parsed from the
        binary file of export_ply(binary=True), in the order of patches()."""
        data = self.export_ply(binary=True)
        end = data.index(b"end_header\n") + len(b"end_header\n")
        n = int(data[:end].split(b"element vertex ")[1].split(b"\n")[0])
        return np.frombuffer(data, dtype=PLY_VERTEX_DTYPE, count=n, offset=end).copy()

    # ---- dense maps and fusion
    def _maps_config(self, source, min_consistent, depth_tol, normal_cos, dedupe):
        c = MapsConfig()
        self.L.mvs_default_maps_config(C.byref(c))
        c.source, c.min_consistent, c.depth_tol, c.normal_cos, c.dedupe = int(source), int(min_consistent), float(depth_tol), float(normal_cos), int(dedupe)
        return c

    def level_shape(self, v):
        """(H, W) of view v at the engine's level: the shape of its dense maps"""
        w, h = C.c_int(), C.c_int()
        self._check(self.L.mvs_engine_get_pyramid(self.h, v, self.cfg.level, None, C.byref(w), C.byref(h)))
        return h.value, w.value

    def render_maps(self, source=0, depth_tol=0.01, normal_cos=0.9, views=None):
        """The dense maps of every view at the engine's level (include/mvskit_engine.h, mvs_engine_render_maps): a list with one dict per
        view -- depth [H, W] float32, normal [H, W, 3], conf [H, W], ids [H, W] int32 (-1: invalid; NaN in the float maps there) and
        agree [H, W] uint64 (bit u: view u agrees) -- or None for a view that `views` (default: all) does not list.  source 0: the
        best-NCC patch of each cell among those with that reference view; 1: the cell's depth-map patch.  Reads engine state only."""
        n = self.cfg.nviews
        want = range(n) if views is None else [int(v) for v in views]
        if any(v < 0 or v >= n for v in want):
            raise ValueError(f"render_maps: views must lie in 0..{n - 1}")
        c = self._maps_config(source, 0, depth_tol, normal_cos, 1)
        slots = (ViewMaps * n)()
        res = [None] * n
        for v in want:
            h, w = self.level_shape(v)
            res[v] = {"depth": np.zeros((h, w), np.float32), "normal": np.zeros((h, w, 3), np.float32), "conf": np.zeros((h, w), np.float32),
                      "ids": np.zeros((h, w), np.int32), "agree": np.zeros((h, w), np.uint64)}
            for k, a in res[v].items():
                setattr(slots[v], k, a.ctypes.data)
        self._check(self.L.mvs_engine_render_maps(self.h, C.byref(c), slots, None))
        return res

    def valid_pixels(self, source=0):
        """the number of valid pixels of every view's dense map (int64 per view), without downloading a map"""
        c = self._maps_config(source, 0, 0.01, 0.9, 1)
        out = np.zeros(self.cfg.nviews, np.int64)
        self._check(self.L.mvs_engine_render_maps(self.h, C.byref(c), None, _ptr(out)))
        return out

    def fused_points(self, source=0, min_consistent=1, depth_tol=0.01, normal_cos=0.9, dedupe=True):
        """The dense point cloud of the pixels that at least `min_consistent` other views agree with (include/mvskit_engine.h,
        mvs_engine_fused_points), as a FUSED_POINT_DTYPE array in (view, y, x) order; with dedupe only the lowest view of an agreeing set
        emits.  Makes the size call first.  Reads engine state only."""
        c = self._maps_config(source, min_consistent, depth_tol, normal_cos, 1 if dedupe else 0)
        n = C.c_int64()
        self._check(self.L.mvs_engine_fused_points(self.h, C.byref(c), 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=FUSED_POINT_DTYPE)
        if n.value:
            self._check(self.L.mvs_engine_fused_points(self.h, C.byref(c), n.value, _ptr(out), C.byref(n)))
        return out[:n.value]

    # ---- triangle mesh
    def tsdf(self, volume, source=0, min_consistent=1, depth_tol=0.01, normal_cos=0.9):
        """The truncated signed distance of every lattice point of `volume` to the dense maps' planes, averaged over the views that see
        it (include/mvskit_engine.h, mvs_engine_tsdf): (tsdf [nz, ny, nx] float32, NaN where no view contributed; count, int32).  Reads
        engine state only."""
        c = self._maps_config(source, min_consistent, depth_tol, normal_cos, 0)
        tsdf, count = np.zeros(volume.shape, np.float32), np.zeros(volume.shape, np.int32)
        self._check(self.L.mvs_engine_tsdf(self.h, C.byref(c), C.byref(volume), _ptr(tsdf), _ptr(count)))
        return tsdf, count

    def _mesh(self, call, cap_v=0, cap_t=0, always=False):
        """-> (verts [n, 3] float32, tris [m, 3] int32).  With estimated caps the full call comes first, and only a mesh that does not fit
        them (MVS_ERR_CAPACITY leaves the exact counts) is run again; without, the size call comes first.  An empty mesh is not asked for
        a second time unless `always`."""
        nv, nt = C.c_int64(), C.c_int64()
        if cap_v > 0 and cap_t > 0:
            verts, tris = np.zeros((cap_v, 3), np.float32), np.zeros((cap_t, 3), np.int32)
            status = call(cap_v, _ptr(verts), cap_t, _ptr(tris), C.byref(nv), C.byref(nt))
            if status == 0:
                return verts[:nv.value].copy(), tris[:nt.value].copy()
            if status != MVS_ERR_CAPACITY:
                self._check(status)
        else:
            self._check(call(0, None, 0, None, C.byref(nv), C.byref(nt)))
        verts, tris = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
        if always or nv.value or nt.value:
            self._check(call(nv.value, _ptr(verts), nt.value, _ptr(tris), C.byref(nv), C.byref(nt)))
        return verts, tris

    def _mesh_vmap(self, fn, params, verts, tris):
        """prune_mesh / decimate_mesh -> (verts, tris, vmap): the size call without vmap, then always the full call, vmap preset to -1"""
        vmap = np.full(verts.shape[0], -1, np.int32)
        head = (self.h, C.byref(params), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris))
        out_v, out_t = self._mesh(lambda cap_v, pv, cap_t, pt, *n: fn(*head, cap_v, pv, cap_t, pt, None if pv is None else _ptr(vmap), *n), always=True)
        return out_v, out_t, vmap

    def extract_mesh(self, volume, tsdf, count=None):
        """Marching tetrahedra over a volume (include/mvskit_engine.h, mvs_engine_extract_mesh): (verts [n, 3] float32, tris [m, 3] int32),
        the triangles facing from negative to positive values.  A lattice point counts when its value is not NaN and, with `count`, count
        >= volume.min_count.  Needs no views."""
        tsdf = np.ascontiguousarray(tsdf, dtype=np.float32)
        count = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
        if tsdf.size != np.prod(volume.shape) or (count is not None and count.size != tsdf.size):
            raise ValueError("extract_mesh: tsdf and count must have one value per lattice point")
        return self._mesh(lambda *a: self.L.mvs_engine_extract_mesh(self.h, C.byref(volume), _ptr(tsdf), _ptr(count), *a))

    def mesh(self, volume, source=0, min_consistent=1, depth_tol=0.01, normal_cos=0.9, cap_v=0, cap_t=0):
        """extract_mesh(volume, *tsdf(volume, ...)) with the volume staying on the device (mvs_engine_mesh): the same arrays.  Every
        call of mvs_engine_mesh fuses the volume, the size call too: with estimates cap_v and cap_t (vertices, triangles) that hold the
        mesh the volume is fused once; estimates that prove too small cost one more call."""
        c = self._maps_config(source, min_consistent, depth_tol, normal_cos, 0)
        return self._mesh(lambda *a: self.L.mvs_engine_mesh(self.h, C.byref(c), C.byref(volume), *a), int(cap_v), int(cap_t))

    # ---- vertex normals and colours of a mesh
    def mesh_normals(self, verts, tris):
        """Area-weighted vertex normals of the mesh verts [n, 3], tris [m, 3] (include/mvskit_engine.h, mvs_engine_mesh_normals): float32
        [n, 3], unit length, zero for a vertex that no triangle with an area uses.  An order-free integer sum: the same bytes whatever
        order the triangles are listed in.  Needs no views."""
        verts, tris = _verts(verts), _tris(tris)
        out = np.zeros((verts.shape[0], 3), np.float32)
        self._check(self.L.mvs_engine_mesh_normals(self.h, verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(out)))
        return out

    def mesh_colours(self, verts, normals=None, source=0, min_consistent=1, depth_tol=0.01, normal_cos=0.9, occl_tol=0.01, min_cos=0.1, visible=None):
        """A colour per vertex from the views that see it (include/mvskit_engine.h, mvs_engine_mesh_colours): (rgb [n, 3] uint8, used [n]
        uint8).  A view counts when the vertex projects into its sampling window (and foreground), faces it (normal . ray >= min_cos; no
        test without normals or for a zero normal) and is not contradicted by the view's dense map (a usable pixel whose plane lies more
        than occl_tol, relative, before or behind the vertex).  Views whose map confirms the vertex are blended if there are any (used =
        their number | 0x80), otherwise the views whose map says nothing there (used = their number); grey and 0 with no view at all.
        visible: a uint64 per vertex (mesh_visibility's, or the caller's); view v then counts for vertex i only when bit v of visible[i]
        is set (mvs_engine_mesh_colours_visible).  Reads engine state only."""
        verts = _verts(verts)
        if normals is not None:
            normals = _verts(normals)
            if normals.shape != verts.shape:
                raise ValueError("mesh_colours: one normal per vertex")
        c = self._maps_config(source, min_consistent, depth_tol, normal_cos, 0)
        m = MeshColouring(float(occl_tol), float(min_cos))
        rgb, used = np.zeros((verts.shape[0], 3), np.uint8), np.zeros(verts.shape[0], np.uint8)
        if visible is None:
            self._check(self.L.mvs_engine_mesh_colours(self.h, C.byref(c), C.byref(m), verts.shape[0], _ptr(verts), _ptr(normals), _ptr(rgb), _ptr(used)))
            return rgb, used
        visible = np.ascontiguousarray(visible, dtype=np.uint64).reshape(-1)
        if visible.shape[0] != verts.shape[0]:
            raise ValueError("mesh_colours: one visibility word per vertex")
        self._check(self.L.mvs_engine_mesh_colours_visible(self.h, C.byref(c), C.byref(m), verts.shape[0], _ptr(verts), _ptr(normals), _ptr(visible), _ptr(rgb),
                                                           _ptr(used)))
        return rgb, used

    # ---- the mesh seen from the views
    def render_mesh(self, verts, tris, views=None):
        """The mesh rasterised into the views at the engine's level (include/mvskit_engine.h, mvs_engine_mesh_render): (maps, covered,
        skipped) -- maps a list with one (depth [H, W] float32, tri [H, W] int32) per view, the depth of the nearest triangle at each
        pixel centre and its row in tris (NaN and -1 where none covers it), or None for a view that `views` (default: all) does not list;
        covered [nviews] int64, the pixels with a triangle; skipped [nviews] int64, the triangles with a vertex behind the camera, not
        finite or beyond 2^16 pixels (there is no near-plane clipping).  Both faces render, masks play no part.  An order-free minimum:
        the same bytes whatever order the triangles are listed in.  Needs views but no pool."""
        verts, tris = _verts(verts), _tris(tris)
        n = self.cfg.nviews
        want = range(n) if views is None else [int(v) for v in views]
        if any(v < 0 or v >= n for v in want):
            raise ValueError(f"render_mesh: views must lie in 0..{n - 1}")
        slots = (MeshViewRender * n)()
        maps = [None] * n
        for v in want:
            h, w = self.level_shape(v)
            maps[v] = (np.zeros((h, w), np.float32), np.zeros((h, w), np.int32))
            slots[v].depth, slots[v].tri = maps[v][0].ctypes.data, maps[v][1].ctypes.data
        covered, skipped = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self._check(self.L.mvs_engine_mesh_render(self.h, verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), slots, None, None, _ptr(covered),
                                                  _ptr(skipped)))
        return maps, covered, skipped

    def mesh_screen(self, verts, tris):
        """What the render sees of every vertex (mvs_engine_mesh_render's screen and vdepth): (screen [nviews, n, 2] int32, the position
        in 1/256 pixel; vdepth [nviews, n] float32, the depth along the optical axis).  A vertex is usable in a view when its depth is
        positive and finite and |screen| <= 2^24."""
        verts, tris = _verts(verts), _tris(tris)
        n = self.cfg.nviews
        screen, vdepth = np.zeros((n, verts.shape[0], 2), np.int32), np.zeros((n, verts.shape[0]), np.float32)
        self._check(self.L.mvs_engine_mesh_render(self.h, verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), None, _ptr(screen), _ptr(vdepth), None, None))
        return screen, vdepth

    def mesh_render_lists(self, verts, tris):
        """Per view the triangles of the mesh that the render hands to its wave-per-triangle kernel, a clipped bounding box of more than
        32 pixel centres (mvs_engine_mesh_render_lists): int64 [nviews], counted on the device.  The others are rasterised a lane each."""
        verts, tris = _verts(verts), _tris(tris)
        out = np.zeros(self.cfg.nviews, np.int64)
        self._check(self.L.mvs_engine_mesh_render_lists(self.h, verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(out)))
        return out

    def mesh_visibility(self, verts, tris, tol=0.01):
        """The views that see each vertex of the mesh (include/mvskit_engine.h, mvs_engine_mesh_visibility): uint64 [n], bit v set when the
        vertex is usable in view v, its nearest pixel lies inside the image and the mesh rendered there is not nearer than the vertex by
        more than `tol`, relative (an empty pixel hides nothing).  What mesh_colours(visible=) takes.  Needs views but no pool."""
        verts, tris = _verts(verts), _tris(tris)
        out = np.zeros(verts.shape[0], np.uint64)
        self._check(self.L.mvs_engine_mesh_visibility(self.h, float(tol), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(out)))
        return out

    # ---- textured mesh
    def mesh_face_views(self, verts, tris, visible=None, front_only=True):
        """The view that textures each triangle (include/mvskit_texture.h, mvs_engine_mesh_face_views): (label [m] int32, the view in
        which the triangle projects largest among those where its three vertices are usable and inside the bilinear window, it has an
        area, faces the camera (front_only) and -- with visible, mesh_visibility's words -- all three vertices are seen; -1 when there
        is none, the lowest view among equals; area [m] int64, the winner's |area| in 1/65536 pixel^2; n_faces [nviews] int64, the
        triangles per label).  Needs views but no pool."""
        verts, tris = _verts(verts), _tris(tris)
        if visible is not None:
            visible = np.ascontiguousarray(visible, dtype=np.uint64).reshape(-1)
            if visible.shape[0] != verts.shape[0]:
                raise ValueError("mesh_face_views: one visibility word per vertex")
        x = MeshTexturing(8, 4096, int(bool(front_only)), 0)
        label, area, faces = np.zeros(tris.shape[0], np.int32), np.zeros(tris.shape[0], np.int64), np.zeros(self.cfg.nviews, np.int64)
        self._check(self.L.mvs_engine_mesh_face_views(self.h, C.byref(x), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(visible), _ptr(label),
                                                      _ptr(area), _ptr(faces)))
        return label, area, faces

    def texture_mesh(self, verts, tris, label, res=8, width=4096):
        """The texture atlas of the mesh under `label` (include/mvskit_texture.h, mvs_engine_mesh_texture): (atlas [H, width, 3] uint8,
        uv [m, 3, 2] int32, the (column, row) of the texel under each corner; the number of textured triangles).  Every triangle whose
        label is honoured (its vertices usable in that view, an area there) gets half a cell of res + 3 texels, sampled from the view at
        the engine's level at the perspective-correct position; the others point at the grey cell 0.  The size call comes first."""
        verts, tris = _verts(verts), _tris(tris)
        label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
        if label.shape[0] != tris.shape[0]:
            raise ValueError("texture_mesh: one label per triangle")
        x = MeshTexturing(int(res), int(width), 1, 0)
        h, n = C.c_int64(), C.c_int64()
        head = (self.h, C.byref(x), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(label))
        self._check(self.L.mvs_engine_mesh_texture(*head, 0, None, None, C.byref(h), C.byref(n)))
        atlas, uv = np.zeros((h.value, int(width), 3), np.uint8), np.zeros((tris.shape[0], 3, 2), np.int32)
        self._check(self.L.mvs_engine_mesh_texture(*head, h.value, _ptr(atlas), _ptr(uv), C.byref(h), C.byref(n)))
        return atlas, uv, n.value

    # ---- seams of the textured mesh
    def mesh_adjacency(self, n_v, tris):
        """The triangle across each edge (include/mvskit_seams.h, mvs_engine_mesh_adjacency): (nbr [m, 3] int32, nbr[t][k] the row of the
        triangle that has the reverse of t's edge from vertex k to vertex (k + 1) % 3 when both directed edges occur once, else -1; the
        number of irregular edges, as mesh_boundaries counts them).  Needs no views."""
        tris = _tris(tris)
        nbr, ni = np.zeros((tris.shape[0], 3), np.int32), C.c_int64()
        self._check(self.L.mvs_engine_mesh_adjacency(self.h, int(n_v), tris.shape[0], _ptr(tris), _ptr(nbr), C.byref(ni)))
        return nbr, ni.value

    def mesh_face_quality(self, verts, tris, visible=None, front_only=True):
        """How well each view shows each triangle (include/mvskit_seams.h, mvs_engine_mesh_face_quality): uint8 [m, nviews], 0 where the
        view is no candidate under mesh_face_views' gates, else max(1, 255 |area| // the triangle's largest |area|): mesh_face_views'
        winner has 255.  Needs views but no pool."""
        verts, tris = _verts(verts), _tris(tris)
        if visible is not None:
            visible = np.ascontiguousarray(visible, dtype=np.uint64).reshape(-1)
            if visible.shape[0] != verts.shape[0]:
                raise ValueError("mesh_face_quality: one visibility word per vertex")
        x = MeshTexturing(8, 4096, int(bool(front_only)), 0)
        quality = np.zeros((tris.shape[0], self.cfg.nviews), np.uint8)
        self._check(self.L.mvs_engine_mesh_face_quality(self.h, C.byref(x), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(visible),
                                                        _ptr(quality)))
        return quality

    def smooth_face_views(self, tris, quality, label, keep=192, iterations=64):
        """The view labels with fewer changes of view across edges (include/mvskit_seams.h, mvs_engine_mesh_smooth_labels): (label [m]
        int32, stats [4] int64 = seams before, seams after, moves, iterations that moved something).  A triangle moves to the label of
        its neighbours that agrees with more of them than its own, among the views whose quality for it is at least `keep`; the movers
        of an iteration are an independent set.  Needs no views."""
        tris = _tris(tris)
        quality = np.ascontiguousarray(quality, dtype=np.uint8)
        label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
        if quality.ndim != 2 or quality.shape[0] != tris.shape[0] or label.shape[0] != tris.shape[0]:
            raise ValueError("smooth_face_views: one row of quality and one label per triangle")
        s = MeshSeams(int(keep), int(iterations), 32, 4)
        out, stats = np.zeros(tris.shape[0], np.int32), np.zeros(4, np.int64)
        n_v = int(tris.max()) + 1 if tris.size else 0
        self._check(self.L.mvs_engine_mesh_smooth_labels(self.h, C.byref(s), max(n_v, 0), tris.shape[0], _ptr(tris), quality.shape[1], _ptr(quality),
                                                         _ptr(label), _ptr(out), _ptr(stats)))
        return out, stats

    def seam_levels(self, verts, tris, label, max_shift=32, samples=4):
        """The views' colour levels from the seams (include/mvskit_seams.h, mvs_engine_mesh_seam_levels): (offset [nviews, 3] int32 in
        1/16 grey level, what texture_mesh_levelled adds to a view's texels; pairs [nviews, nviews, 4] int64, per pair of views the
        samples on the seam edges between them and the summed differences of the three channels in 1/16 grey level; the number of seam
        edges).  Needs views but no pool."""
        verts, tris = _verts(verts), _tris(tris)
        label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
        if label.shape[0] != tris.shape[0]:
            raise ValueError("seam_levels: one label per triangle")
        n = self.cfg.nviews
        s, x = MeshSeams(192, 64, int(max_shift), int(samples)), MeshTexturing(8, 4096, 1, 0)
        offset, pairs, ne = np.zeros((n, 3), np.int32), np.zeros((n, n, 4), np.int64), C.c_int64()
        self._check(self.L.mvs_engine_mesh_seam_levels(self.h, C.byref(s), C.byref(x), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(label),
                                                       _ptr(offset), _ptr(pairs), C.byref(ne)))
        return offset, pairs, ne.value

    def texture_mesh_levelled(self, verts, tris, label, offset, res=8, width=4096):
        """texture_mesh with `offset` [nviews, 3] (seam_levels'; None: zeros) added to the texels of each view before they are rounded
        (include/mvskit_seams.h, mvs_engine_mesh_texture_levelled): (atlas, uv, the number of textured triangles)."""
        verts, tris = _verts(verts), _tris(tris)
        label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
        if label.shape[0] != tris.shape[0]:
            raise ValueError("texture_mesh_levelled: one label per triangle")
        if offset is not None:
            offset = np.ascontiguousarray(offset, dtype=np.int32)
            if offset.shape != (self.cfg.nviews, 3):
                raise ValueError("texture_mesh_levelled: offset is [nviews, 3]")
        x = MeshTexturing(int(res), int(width), 1, 0)
        h, n = C.c_int64(), C.c_int64()
        head = (self.h, C.byref(x), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(label), _ptr(offset))
        self._check(self.L.mvs_engine_mesh_texture_levelled(*head, 0, None, None, C.byref(h), C.byref(n)))
        atlas, uv = np.zeros((h.value, int(width), 3), np.uint8), np.zeros((tris.shape[0], 3, 2), np.int32)
        self._check(self.L.mvs_engine_mesh_texture_levelled(*head, h.value, _ptr(atlas), _ptr(uv), C.byref(h), C.byref(n)))
        return atlas, uv, n.value

    def textured_mesh(self, volume, source=0, min_consistent=1, depth_tol=0.01, normal_cos=0.9, cap_v=0, cap_t=0, min_triangles=0, largest_only=False,
                      smooth_iterations=0, decimate_cell=0.0, decimate_placement="mean", fill_max_edges=0, res=8, atlas_width=4096, front_only=True,
                      visibility_tol=0.01, seam_keep=0, level_colours=False):
        """mesh, the clean-up steps of coloured_mesh in its order (prune, fill, smooth, decimate), mesh_normals, mesh_visibility,
        mesh_face_views and texture_mesh chained: (verts, tris, normals, atlas, uv, label), what write_mesh_obj takes.  seam_keep in
        1..255: the labels go through mesh_face_quality and smooth_face_views(keep=seam_keep) first; level_colours: the atlas is
        texture_mesh_levelled's under seam_levels' offsets."""
        kw = dict(source=source, min_consistent=min_consistent, depth_tol=depth_tol, normal_cos=normal_cos)
        verts, tris = self.mesh(volume, cap_v=cap_v, cap_t=cap_t, **kw)
        if min_triangles > 0 or largest_only:
            verts, tris, _ = self.prune_mesh(verts, tris, max(1, int(min_triangles)), largest_only)
        if fill_max_edges >= 3:
            verts, tris, _ = self.fill_holes(verts, tris, fill_max_edges)
        if smooth_iterations > 0:
            verts = self.smooth_mesh(verts, tris, smooth_iterations)
        if decimate_cell > 0:
            verts, tris, _ = self.decimate_mesh(verts, tris, decimate_cell, decimation_origin(volume), decimate_placement)
        normals = self.mesh_normals(verts, tris)
        visible = self.mesh_visibility(verts, tris, visibility_tol)
        label, _, _ = self.mesh_face_views(verts, tris, visible=visible, front_only=front_only)
        if seam_keep > 0:
            quality = self.mesh_face_quality(verts, tris, visible=visible, front_only=front_only)
            label, _ = self.smooth_face_views(tris, quality, label, keep=seam_keep)
        if level_colours:
            offset, _, _ = self.seam_levels(verts, tris, label)
            atlas, uv, _ = self.texture_mesh_levelled(verts, tris, label, offset, res=res, width=atlas_width)
        else:
            atlas, uv, _ = self.texture_mesh(verts, tris, label, res=res, width=atlas_width)
        return verts, tris, normals, atlas, uv, label

    # ---- mesh clean-up
    def mesh_components(self, n_v, tris):
        """The connected components of the mesh's vertex graph (include/mvskit_engine.h, mvs_engine_mesh_components): (label [n_v] int32,
        the smallest vertex id of each vertex's component; ntris [n_v] int32, the triangles of that component; the number of components
        with a triangle).  Needs no views."""
        tris = _tris(tris)
        label, ntris, n = np.zeros(int(n_v), np.int32), np.zeros(int(n_v), np.int32), C.c_int64()
        self._check(self.L.mvs_engine_mesh_components(self.h, int(n_v), tris.shape[0], _ptr(tris), _ptr(label), _ptr(ntris), C.byref(n)))
        return label, ntris, n.value

    def prune_mesh(self, verts, tris, min_triangles=1, largest_only=False):
        """The mesh without the components of fewer than min_triangles triangles (largest_only: without all but the largest) and without
        the vertices that no kept triangle names (include/mvskit_engine.h, mvs_engine_mesh_prune): (verts, tris, vmap [n] int32, the new
        id of every input vertex or -1).  What stays keeps its order and its bytes.  The size call comes first.  Needs no views."""
        verts, tris = _verts(verts), _tris(tris)
        return self._mesh_vmap(self.L.mvs_engine_mesh_prune, MeshPruning(int(min_triangles), int(bool(largest_only)), 0), verts, tris)

    def smooth_mesh(self, verts, tris, iterations=10, lam=0.5, mu=-0.53):
        """Taubin smoothing of the positions (include/mvskit_engine.h, mvs_engine_mesh_smooth): float32 [n, 3].  Every iteration moves
        each vertex by lam towards the mean of its triangles' other corners and then, unless mu is 0, by mu away from it again; an
        order-free integer sum, the same bytes whatever order the triangles are listed in.  Boundaries are not pinned.  Needs no views."""
        verts, tris = _verts(verts), _tris(tris)
        s = MeshSmoothing(int(iterations), float(lam), float(mu), 0)
        out = np.zeros((verts.shape[0], 3), np.float32)
        self._check(self.L.mvs_engine_mesh_smooth(self.h, C.byref(s), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), _ptr(out)))
        return out

    # ---- mesh decimation
    def decimate_mesh(self, verts, tris, cell, origin=(0.0, 0.0, 0.0), placement="mean"):
        """Vertex clustering on the grid of edge `cell` with a corner at `origin` (include/mvskit_engine.h, mvs_engine_mesh_decimate):
        (verts, tris, vmap [n] int32, the output id of every input vertex's cluster or -1).  One vertex per occupied cell, at the mean of
        the cell's vertices (placement "mean") or at the one of them nearest to that mean ("member"); triangles that no longer join
        three cells go, and of those that join the same three only the first stays.  The result of a closed surface need not be closed.
        The same bytes whatever order the hardware meets the triangles in.  The size call comes first.  Needs no views."""
        verts, tris = _verts(verts), _tris(tris)
        if placement not in ("mean", "member"):
            raise ValueError("decimate_mesh: placement is 'mean' or 'member'")
        d = MeshDecimation((C.c_float * 3)(*[float(o) for o in origin]), float(cell), 1 if placement == "member" else 0, 0)
        return self._mesh_vmap(self.L.mvs_engine_mesh_decimate, d, verts, tris)

    # ---- mesh hole filling
    def mesh_boundaries(self, n_v, tris):
        """The boundary loops of the mesh (include/mvskit_engine.h, mvs_engine_mesh_boundaries): (loop [n_v] int32, the smallest vertex id
        of each vertex's boundary component or -1; length [n_v] int32, the half-edges of that component, negated when it is no simple
        loop; the numbers of loops, of complex components and of irregular edges).  A mesh is a closed edge-manifold exactly when the
        three counts are 0.  Needs no views."""
        tris = _tris(tris)
        loop, length = np.zeros(int(n_v), np.int32), np.zeros(int(n_v), np.int32)
        nl, nc, ni = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.L.mvs_engine_mesh_boundaries(self.h, int(n_v), tris.shape[0], _ptr(tris), _ptr(loop), _ptr(length), C.byref(nl), C.byref(nc),
                                                      C.byref(ni)))
        return loop, length, nl.value, nc.value, ni.value

    def fill_holes(self, verts, tris, max_edges=64):
        """The mesh with its boundary loops of 3 .. max_edges edges closed (include/mvskit_engine.h, mvs_engine_mesh_fill): (verts, tris,
        the number of loops filled).  A loop of 3 gets its triangle back; a longer one a new vertex at its centroid and a fan around
        it.  The input rows stay where they are, the new ones follow them; ids do not change.  The rim of an open surface is a loop too:
        max_edges keeps it open.  The same bytes whatever order the hardware meets the triangles in.  The size call comes first.  Needs
        no views."""
        verts, tris = _verts(verts), _tris(tris)
        f = MeshFilling(int(max_edges), 0)
        nf = C.c_int64()
        out_v, out_t = self._mesh(lambda *a: self.L.mvs_engine_mesh_fill(self.h, C.byref(f), verts.shape[0], _ptr(verts), tris.shape[0], _ptr(tris), *a,
                                                                         C.byref(nf)))
        return out_v, out_t, nf.value

    def coloured_mesh(self, volume, source=0, min_consistent=1, depth_tol=0.01, normal_cos=0.9, occl_tol=0.01, min_cos=0.1, cap_v=0, cap_t=0,
                      min_triangles=0, largest_only=False, smooth_iterations=0, decimate_cell=0.0, decimate_placement="mean", fill_max_edges=0,
                      mesh_occlusion=False, visibility_tol=0.01):
        """mesh, mesh_normals and mesh_colours chained: (verts, tris, normals, rgb, used), what write_mesh_ply takes.  Every step renders
        the maps it needs itself.  With min_triangles >= 1 or largest_only the mesh is pruned (prune_mesh), with fill_max_edges >= 3 its
        holes of up to that many edges are filled (fill_holes: the floaters are gone first, and the smoothing relaxes the fans), with
        smooth_iterations > 0 it is smoothed (smooth_mesh with its default steps), with decimate_cell > 0 decimated (decimate_mesh), in
        that order, before the normals and colours are taken.  The decimation grid starts at volume.origin - voxel / 2: marching tetrahedra leaves lattice coordinates in
        two of a vertex's three components, and with a cell that is a multiple of the voxel none of them sits on a cell boundary.
        mesh_occlusion: the colours also take the visibility of the final mesh (mesh_visibility with visibility_tol, behind the
        decimation) -- a view that looks at a vertex through the front of the mesh no longer colours it; False calls nothing new."""
        kw = dict(source=source, min_consistent=min_consistent, depth_tol=depth_tol, normal_cos=normal_cos)
        verts, tris = self.mesh(volume, cap_v=cap_v, cap_t=cap_t, **kw)
        if min_triangles > 0 or largest_only:
            verts, tris, _ = self.prune_mesh(verts, tris, max(1, int(min_triangles)), largest_only)
        if fill_max_edges >= 3:
            verts, tris, _ = self.fill_holes(verts, tris, fill_max_edges)
        if smooth_iterations > 0:
            verts = self.smooth_mesh(verts, tris, smooth_iterations)
        if decimate_cell > 0:
            verts, tris, _ = self.decimate_mesh(verts, tris, decimate_cell, decimation_origin(volume), decimate_placement)
        normals = self.mesh_normals(verts, tris)
        visible = self.mesh_visibility(verts, tris, visibility_tol) if mesh_occlusion else None
        rgb, used = self.mesh_colours(verts, normals, occl_tol=occl_tol, min_cos=min_cos, visible=visible, **kw)
        return verts, tris, normals, rgb, used

    # ---- the hot path
    def propagate(self, it):
        c = Counters()
        self._check(self.L.mvs_engine_propagate(self.h, it, C.byref(c)))
        return c.as_dict()

    def filter(self):
        r = np.zeros(4, dtype=np.int64)
        self._check(self.L.mvs_engine_filter(self.h, _ptr(r)))
        return {"outside": int(r[0]), "exact": int(r[1]), "neighbor": int(r[2]), "groups": int(r[3])}

    def filter_stats(self):
        f = FilterStats()
        self._check(self.L.mvs_engine_filter_stats(self.h, C.byref(f)))
        return _record(f)

    def engine_pass(self, it, p):
        c = Counters()
        self._check(self.L.mvs_engine_pass(self.h, it, p, C.byref(c)))
        return c.as_dict()

    def export_counts(self):
        a, b = C.c_int64(), C.c_int64()
        pv = np.zeros(self.cfg.nviews, dtype=np.int32)
        self._check(self.L.mvs_engine_export_counts(self.h, C.byref(a), C.byref(b), _ptr(pv)))
        return a.value, b.value, pv

    def export_device(self, new_ptr, cap_new, kill_ptr, cap_kill):
        self._check(self.L.mvs_engine_export_device(self.h, new_ptr, cap_new, kill_ptr, cap_kill))

    def commit_device(self, new_ptr, n_new, kill_ptr, n_kill):
        self._check(self.L.mvs_engine_commit_device(self.h, new_ptr, n_new, kill_ptr, n_kill))

    def commit_local(self):
        self._check(self.L.mvs_engine_commit_local(self.h))

    # ---- multi-GPU (RCCL communicator inside the engine)
    COMM_ID_BYTES = 128

    def comm_unique_id(self):
        """ncclGetUniqueId as bytes; rank 0 calls it and hands the bytes to the other ranks."""
        buf = C.create_string_buffer(self.COMM_ID_BYTES)
        self._check(self.L.mvs_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int):
        assert len(uid) == self.COMM_ID_BYTES
        self._check(self.L.mvs_engine_comm_init(self.h, C.c_char_p(uid), rank, world))

    def comm_info(self):
        """rank / world the engine holds and what its communicator reports (ncclCommCount / ncclCommUserRank; -1 if it cannot be asked)"""
        r, w, cc, cr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.mvs_engine_comm_info(self.h, C.byref(r), C.byref(w), C.byref(cc), C.byref(cr)))
        return {"rank": r.value, "world": w.value, "comm_count": cc.value, "comm_rank": cr.value}

    def comm_release(self):
        self._check(self.L.mvs_engine_comm_release(self.h))

    def exchange(self):
        self._check(self.L.mvs_engine_exchange(self.h))

    def timing(self):
        t = Timing()
        self._check(self.L.mvs_engine_last_timing(self.h, C.byref(t)))
        return _record(t)

    def _counts(self, fn, keys):
        """the `int64_t out[N]` counters of fn under their keys"""
        out = (C.c_int64 * len(keys))()
        self._check(fn(self.h, out))
        return dict(zip(keys, (int(x) for x in out)))

    #: mvs_engine_sweep_pairs: the sweep's trials by how they were refined, since the engine was created
    SWEEP_PAIR_KEYS = ("paired", "alone_no_partner", "alone_no_room", "alone_partner_failed", "alone_long_list", "can_pair")

    def sweep_pairs(self):
        return self._counts(self.L.mvs_engine_sweep_pairs, self.SWEEP_PAIR_KEYS)

    #: mvs_engine_sweep_repeats: the trials of full cells that did not run again what the trial before them had computed
    SWEEP_REPEAT_KEYS = ("skipped", "from_stash")

    def sweep_repeats(self):
        return self._counts(self.L.mvs_engine_sweep_repeats, self.SWEEP_REPEAT_KEYS)

    #: mvs_engine_sweep_kernels: sweep launches by the kernel the launcher chose, since the engine was created
    SWEEP_KERNEL_KEYS = ("generic", "full_window")

    def sweep_kernels(self):
        return self._counts(self.L.mvs_engine_sweep_kernels, self.SWEEP_KERNEL_KEYS)

    #: mvs_engine_sampler_launches: sweep launches and refine probes by the form of their texture samplers, since the engine was created
    SAMPLER_LAUNCH_KEYS = ("sweep_wide", "sweep_narrow", "refine_wide", "refine_narrow")

    def sampler_launches(self):
        return self._counts(self.L.mvs_engine_sampler_launches, self.SAMPLER_LAUNCH_KEYS)

    def depth_normal_map(self, view, kind):
        gw, gh = self.grid_dims(view)
        d = np.zeros((gh, gw), np.float32)
        n = np.zeros((gh, gw, 3), np.float32)
        ids = np.zeros((gh, gw), np.int32)
        self._check(self.L.mvs_engine_depth_normal_map(self.h, view, kind, _ptr(d), _ptr(n), _ptr(ids)))
        return d, n, ids

    # ---- batched single functions
    def probe(self, op, recs=None, values=None):
        if op == PROBE_MATH:
            x = np.ascontiguousarray(values, dtype=np.float32)
            out = np.zeros((x.shape[0], 5), np.float32)
            self._check(self.L.mvs_engine_probe(self.h, op, x.shape[0], None, _ptr(x), None, _ptr(out), None))
            return out
        recs = synth.convert_records(recs, self.dtype)
        n = recs.shape[0]
        out_rec = np.zeros(n, dtype=self.dtype)
        out_f = np.zeros((n, 4) if op == PROBE_REFINE_X else n, np.float32)  # PROBE_REFINE_X: (x0, x1, x2, cost) per record
        out_i = np.zeros(n, np.int32)
        self._check(self.L.mvs_engine_probe(self.h, op, n, _ptr(recs), None, _ptr(out_rec), _ptr(out_f), _ptr(out_i)))
        return out_rec, out_f, out_i


def make_volume(origin, voxel, dims, trunc, min_count=1):
    """an mvs_volume: lattice point (i, j, k) at origin + (i, j, k) * voxel, dims = (nx, ny, nz)"""
    v = Volume()
    for k in range(3):
        v.origin[k], v.dims[k] = float(origin[k]), int(dims[k])
    v.voxel, v.trunc, v.min_count, v.pad = float(voxel), float(trunc), int(min_count), 0
    return v


def decimation_origin(volume):
    """The grid corner Engine.coloured_mesh gives decimate_mesh: volume.origin - voxel / 2 per component, in float32."""
    half = np.float32(volume.voxel) / np.float32(2)
    return tuple(float(np.float32(volume.origin[k]) - half) for k in range(3))


def volume_around(xyz, voxel, trunc_voxels=4, pad_voxels=2, min_count=1):
    """The mvs_volume of spacing `voxel` around points xyz [n, 3] (those of fused_points(), say): their bounding box with pad_voxels
    lattice points more on every side, trunc = trunc_voxels * voxel."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if xyz.shape[0] == 0 or not np.isfinite(xyz).all() or not voxel > 0:
        raise ValueError("volume_around: needs finite points and a positive voxel")
    lo = xyz.min(axis=0) - pad_voxels * voxel
    dims = np.ceil((xyz.max(axis=0) + pad_voxels * voxel - lo) / voxel).astype(np.int64) + 1
    if (dims < 2).any() or (dims > 1024).any() or int(np.prod(dims)) > 1 << 28:
        raise ValueError(f"volume_around: {dims.tolist()} lattice points: each dimension must lie in 2..1024, their product must not exceed 2^28")
    return make_volume(lo, voxel, dims, trunc_voxels * voxel, min_count)


def write_mesh_ply(path, verts, tris, binary=True, normals=None, colours=None):
    """verts [n, 3] and tris [m, 3] as a PLY file: element vertex (float x, y, z; with normals [n, 3] float nx, ny, nz behind them; with
    colours [n, 3] uchar red, green, blue last) and element face (list uchar int vertex_indices)"""
    verts = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype="<i4").reshape(-1, 3)
    fields, props = [("xyz", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    cols = [verts]
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype="<f4").reshape(-1, 3)
        fields.append(("normal", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
        cols.append(normals)
    if colours is not None:
        colours = np.ascontiguousarray(colours, dtype="u1").reshape(-1, 3)
        fields.append(("rgb", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        cols.append(colours)
    if any(c.shape != verts.shape for c in cols):
        raise ValueError("write_mesh_ply: normals and colours need one row per vertex")
    head = (f"ply\nformat {'binary_little_endian' if binary else 'ascii'} 1.0\nelement vertex {verts.shape[0]}\n{props}"
            f"element face {tris.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if binary:
            faces = np.zeros(tris.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            faces["n"], faces["v"] = 3, tris
            rows = np.zeros(verts.shape[0], dtype=np.dtype(fields))  # packed: 12, 24, 15 or 27 bytes a vertex
            for (name, _, _), c in zip(fields, cols):
                rows[name] = c
            f.write(rows.tobytes())
            f.write(faces.tobytes())
        else:
            lists = [c.tolist() for c in cols]
            f.write("".join(" ".join(f"{x:.9g}" if isinstance(x, float) else str(x) for c in row for x in c) + "\n" for row in zip(*lists)).encode("ascii"))
            f.write("".join(f"3 {a} {b} {c}\n" for a, b, c in tris.tolist()).encode("ascii"))


def encode_png_rgb(image):
    """image [H, W, 3] uint8 as the bytes of an 8-bit RGB PNG: one zlib stream, filter 0 on every row"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("encode_png_rgb: an image of H x W x 3 bytes, H and W at least 1")
    h, w = image.shape[:2]

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    rows = np.zeros((h, 1 + 3 * w), np.uint8)  # the filter byte, 0, in front of every row
    rows[:, 1:] = image.reshape(h, 3 * w)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
            + chunk(b"IEND", b""))


def write_mesh_obj(path, verts, tris, atlas, uv, normals=None):
    """The textured mesh as a Wavefront OBJ at `path`, with a material file and the atlas as an 8-bit RGB PNG beside it (the path's
    stem with .mtl and .png).  atlas [H, W, 3] uint8 and uv [m, 3, 2] int32 texels (column, row) as texture_mesh returns them.  One vt
    per corner, ((column + 0.5) / W, 1 - (row + 0.5) / H): the centre of the texel, v upwards; faces v/vt or, with normals [n, 3],
    v/vt/vn, 1-based."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    atlas = np.ascontiguousarray(atlas, dtype=np.uint8)
    uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 3, 2)
    if uv.shape[0] != tris.shape[0]:
        raise ValueError("write_mesh_obj: three texels per triangle")
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if normals.shape != verts.shape:
            raise ValueError("write_mesh_obj: one normal per vertex")
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    with open(stem + ".png", "wb") as f:
        f.write(encode_png_rgb(atlas))
    with open(stem + ".mtl", "w") as f:
        f.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    H, W = atlas.shape[:2]
    vt = np.stack([(uv[..., 0].astype(np.float64) + 0.5) / W, 1.0 - (uv[..., 1].astype(np.float64) + 0.5) / H], axis=-1).reshape(-1, 2)
    out = [f"mtllib {name}.mtl\n"]
    out += [f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in verts.tolist()]
    if normals is not None:
        out += [f"vn {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in normals.tolist()]
    out += [f"vt {u:.17g} {v:.17g}\n" for u, v in vt.tolist()]
    out.append(f"usemtl {name}\n")
    ids = (tris + 1).tolist()
    if normals is None:
        out += [f"f {a}/{3 * t + 1} {b}/{3 * t + 2} {c}/{3 * t + 3}\n" for t, (a, b, c) in enumerate(ids)]
    else:
        out += [f"f {a}/{3 * t + 1}/{a} {b}/{3 * t + 2}/{b} {c}/{3 * t + 3}/{c}\n" for t, (a, b, c) in enumerate(ids)]
    with open(path, "w") as f:
        f.write("".join(out))
