"""What mirrors include/mvskit_engine.h, once: the constants, the record dtypes, the structs, the signature of every entry point, and
the loader that applies them.  tests/test_abi.py holds SIGNATURES and STRUCTS against the header itself.  The textured-mesh calls of
include/mvskit_texture.h have a table of their own, TEXTURE_SIGNATURES and TEXTURE_STRUCTS, which tests/test_mesh_texture_abi.py holds
against that header in the same way; the seam calls of include/mvskit_seams.h a third, SEAM_SIGNATURES and SEAM_STRUCTS, held by
tests/test_mesh_seams_abi.py."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build

__all__ = ["PROBE_NCC", "PROBE_PREPROCESS", "PROBE_REFINE", "PROBE_POSTPROCESS", "PROBE_COST", "PROBE_MATH", "PROBE_REFINE_X", "REFINE_HALVING",
           "REFINE_CONVERGED", "MVS_OK", "MVS_ERR_ARG", "MVS_ERR_STATE", "MVS_ERR_HIP", "MVS_ERR_CAPACITY", "MVS_ERR_NO_DEVICE", "PLY_ASCII",
           "PLY_BINARY_LE", "PLY_VERTEX_DTYPE", "FUSED_POINT_DTYPE", "Config", "Refiner", "ViewDesc", "SeedView", "SeedRandom", "SeedPoints",
           "MapsConfig", "ViewMaps", "Volume", "MeshColouring", "MeshPruning", "MeshSmoothing", "MeshDecimation", "MeshFilling", "MeshViewRender",
           "MeshTexturing", "TEXTURE_STRUCTS", "TEXTURE_SIGNATURES", "MeshSeams", "SEAM_STRUCTS", "SEAM_SIGNATURES", "Counters", "Timing", "FilterStats", "STRUCTS", "SIGNATURES", "EXPORTS",
           "EngineError", "load_library"]

PROBE_NCC, PROBE_PREPROCESS, PROBE_REFINE, PROBE_POSTPROCESS, PROBE_COST, PROBE_MATH, PROBE_REFINE_X = range(7)
REFINE_HALVING, REFINE_CONVERGED = 0, 1  # mvs_refine_mode
MVS_OK, MVS_ERR_ARG, MVS_ERR_STATE, MVS_ERR_HIP, MVS_ERR_CAPACITY, MVS_ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5  # mvs_status
PLY_ASCII, PLY_BINARY_LE = 0, 1  # mvs_ply_format
#: one vertex of the binary PLY file (mvs_engine_export_ply): 27 packed bytes
PLY_VERTEX_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("normal", "<f4", (3,)), ("rgb", "u1", (3,))])
#: mvs_fused_point: one record of mvs_engine_fused_points, 32 bytes
FUSED_POINT_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("normal", "<f4", (3,)), ("conf", "<f4"), ("rgb", "u1", (3,)), ("view", "u1")])


class Config(C.Structure):
    _fields_ = [("nviews", C.c_int32), ("level", C.c_int32), ("csize", C.c_int32), ("wsize", C.c_int32),
                ("minImageNum", C.c_int32), ("max_propag", C.c_int32), ("nccThreshold", C.c_float),
                ("maxAngleThreshold", C.c_float), ("quadThreshold", C.c_float), ("depth", C.c_int32),
                ("seed", C.c_uint32), ("refine_steps", C.c_int32), ("refine_rd0", C.c_float), ("refine_ra0", C.c_float),
                ("enable_check", C.c_int32), ("view_begin", C.c_int32), ("view_stride", C.c_int32),
                ("device", C.c_int32), ("view_propagation", C.c_int32), ("shard_index", C.c_int32), ("shard_count", C.c_int32),
                ("literal_groups", C.c_int32), ("max_patches", C.c_int64)]


class Refiner(C.Structure):
    """mvs_refiner: which refiner Optim::refinePatch runs (mvs_engine_set_refiner)."""
    _fields_ = [("mode", C.c_int32), ("max_evals", C.c_int32), ("xtol", C.c_float)]


class ViewDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("P", C.c_float * 12), ("rgb", C.c_void_p),
                ("mask", C.c_void_p)]


class SeedView(C.Structure):
    """mvs_seed_view: one view's world-space normal map and level-0 mask (mvs_engine_seed_patches)."""
    _fields_ = [("normals", C.c_void_p), ("mask", C.c_void_p)]


class SeedRandom(C.Structure):
    """mvs_seed_random: the parameters of a cold start (mvs_engine_seed_random); depth_min / depth_max point at one float per view."""
    _fields_ = [("hypotheses", C.c_int32), ("seed", C.c_uint32), ("max_tilt", C.c_float), ("min_ncc", C.c_float),
                ("depth_min", C.c_void_p), ("depth_max", C.c_void_p)]


class SeedPoints(C.Structure):
    """mvs_seed_points: the parameters of a warm start (mvs_engine_seed_points)."""
    _fields_ = [("hypotheses", C.c_int32), ("min_ncc", C.c_float)]


class MapsConfig(C.Structure):
    """mvs_maps_config: the parameters of mvs_engine_render_maps / mvs_engine_fused_points."""
    _fields_ = [("source", C.c_int32), ("min_consistent", C.c_int32), ("depth_tol", C.c_float), ("normal_cos", C.c_float),
                ("dedupe", C.c_int32), ("pad", C.c_int32)]


class ViewMaps(C.Structure):
    """mvs_view_maps: where one view's maps go (host or device pointers, any of them null)."""
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("conf", C.c_void_p), ("ids", C.c_void_p), ("agree", C.c_void_p)]


class Volume(C.Structure):
    """mvs_volume: the lattice of mvs_engine_tsdf / mvs_engine_extract_mesh / mvs_engine_mesh, 40 bytes."""
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("dims", C.c_int32 * 3), ("trunc", C.c_float), ("min_count", C.c_int32),
                ("pad", C.c_int32)]

    @property
    def shape(self):
        """(nz, ny, nx): the shape of the volume's arrays"""
        return self.dims[2], self.dims[1], self.dims[0]


class MeshColouring(C.Structure):
    """mvs_mesh_colouring: the two thresholds of mvs_engine_mesh_colours, 8 bytes."""
    _fields_ = [("occl_tol", C.c_float), ("min_cos", C.c_float)]


class MeshPruning(C.Structure):
    """mvs_mesh_pruning: what mvs_engine_mesh_prune keeps, 16 bytes."""
    _fields_ = [("min_triangles", C.c_int64), ("largest_only", C.c_int32), ("pad", C.c_int32)]


class MeshSmoothing(C.Structure):
    """mvs_mesh_smoothing: the steps of mvs_engine_mesh_smooth, 16 bytes."""
    _fields_ = [("iterations", C.c_int32), ("lam", C.c_float), ("mu", C.c_float), ("pad", C.c_int32)]


class MeshDecimation(C.Structure):
    """mvs_mesh_decimation: the grid and the placement of mvs_engine_mesh_decimate, 24 bytes."""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("placement", C.c_int32), ("pad", C.c_int32)]


class MeshFilling(C.Structure):
    """mvs_mesh_filling: the longest loop mvs_engine_mesh_fill closes, 8 bytes."""
    _fields_ = [("max_edges", C.c_int32), ("pad", C.c_int32)]


class MeshViewRender(C.Structure):
    """mvs_mesh_view_render: where one view's rendered depth and triangle rows go (host or device pointers, either null), 16 bytes."""
    _fields_ = [("depth", C.c_void_p), ("tri", C.c_void_p)]


class MeshTexturing(C.Structure):
    """mvs_mesh_texturing (include/mvskit_texture.h): the atlas of mvs_engine_mesh_face_views / mvs_engine_mesh_texture, 16 bytes."""
    _fields_ = [("res", C.c_int32), ("width", C.c_int32), ("front_only", C.c_int32), ("pad", C.c_int32)]


class MeshSeams(C.Structure):
    """mvs_mesh_seams (include/mvskit_seams.h): the smoothing of the view labels and the levelling on the seams, 16 bytes."""
    _fields_ = [("keep", C.c_int32), ("iterations", C.c_int32), ("max_shift", C.c_int32), ("samples", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("candidates", "prefiltered", "patches", "fail0", "fail1", "inserted",
                                         "replaced", "evals", "view_evals", "trimmed")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Timing(C.Structure):
    _fields_ = [("index_ms", C.c_float), ("sweep_ms", C.c_float), ("commit_ms", C.c_float), ("sweep_launches", C.c_int32),
                ("exchange_ms", C.c_float), ("sweep_jobs_listed", C.c_int32), ("exchange_bytes", C.c_int64), ("check_retried_cells", C.c_int64)]


class FilterStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("outside_ms", "exact_ms", "neighbor_ms", "groups_ms", "rebuild_ms", "total_ms")] + \
               [(n, C.c_int64) for n in ("patches_in", "exact_patches", "exact_view_evals", "neighbor_patches", "neighbor_tasks", "neighbor_entries",
                                         "neighbor_visited", "neighbor_accepted", "neighbor_retried", "exchange_bytes")]


#: the header's name of every struct that has a class here (mvs_patch and mvs_fused_point are numpy dtypes)
STRUCTS = {"mvs_config": Config, "mvs_refiner": Refiner, "mvs_view_desc": ViewDesc, "mvs_counters": Counters, "mvs_seed_view": SeedView,
           "mvs_seed_random": SeedRandom, "mvs_seed_points": SeedPoints, "mvs_maps_config": MapsConfig, "mvs_view_maps": ViewMaps,
           "mvs_volume": Volume, "mvs_mesh_colouring": MeshColouring, "mvs_mesh_pruning": MeshPruning, "mvs_mesh_smoothing": MeshSmoothing,
           "mvs_mesh_decimation": MeshDecimation, "mvs_mesh_filling": MeshFilling, "mvs_mesh_view_render": MeshViewRender,
           "mvs_filter_stats": FilterStats, "mvs_timing": Timing}


def _signatures():
    P, vp, i, i64, f = C.POINTER, C.c_void_p, C.c_int, C.c_int64, C.c_float
    pi, pf, pi64 = P(i), P(f), P(i64)
    cfg, maps, col, vol = P(Config), P(MapsConfig), P(MeshColouring), P(Volume)
    mesh_in = [i64, vp, i64, vp]               # n_v, verts, n_t, tris
    mesh_out = [i64, vp, i64, vp]              # cap_v, out_verts, cap_t, out_tris
    return {
        "mvs_last_error": (C.c_char_p, []),
        "mvs_device_count": (i, []),
        "mvs_list_cap": (i, []),
        "mvs_patch_bytes": (i, []),
        "mvs_default_config": (None, [cfg]),
        "mvs_default_refiner": (None, [P(Refiner)]),
        "mvs_engine_create": (i, [cfg, P(vp)]),
        "mvs_engine_destroy": (i, [vp]),
        "mvs_engine_set_refiner": (i, [vp, P(Refiner)]),
        "mvs_engine_set_views": (i, [vp, i, P(ViewDesc)]),
        "mvs_engine_grid_dims": (i, [vp, i, pi, pi]),
        "mvs_engine_get_pyramid": (i, [vp, i, i, vp, pi, pi]),
        "mvs_engine_set_thresholds": (i, [vp, f, f, i]),
        "mvs_engine_get_thresholds": (i, [vp, pf, pf, pi]),
        "mvs_engine_update_threshold": (i, [vp]),
        "mvs_engine_upload_patches": (i, [vp, i64, vp]),
        "mvs_engine_clear_patches": (i, [vp]),
        "mvs_engine_seed_patches": (i, [vp, i64, vp, P(SeedView), pi64]),
        "mvs_default_seed_random": (None, [P(SeedRandom)]),
        "mvs_engine_seed_random": (i, [vp, P(SeedRandom), pi64]),
        "mvs_engine_seed_random_hypotheses": (i, [vp, P(SeedRandom), i, i64, vp, vp]),
        "mvs_default_seed_points": (None, [P(SeedPoints)]),
        "mvs_engine_seed_points": (i, [vp, P(SeedPoints), i64, vp, pi64]),
        "mvs_engine_seed_points_hypotheses": (i, [vp, P(SeedPoints), i64, vp, vp, vp]),
        "mvs_engine_depth_ranges": (i, [vp, i64, vp, f, vp, vp, vp]),
        "mvs_engine_reserve": (i, [vp, i64]),
        "mvs_engine_num_patches": (i, [vp, pi64]),
        "mvs_engine_download_patches": (i, [vp, i64, vp, pi64]),
        "mvs_engine_export_ply": (i, [vp, i, i64, vp, pi64]),
        "mvs_default_maps_config": (None, [maps]),
        "mvs_engine_render_maps": (i, [vp, maps, P(ViewMaps), vp]),
        "mvs_engine_fused_points": (i, [vp, maps, i64, vp, pi64]),
        "mvs_engine_tsdf": (i, [vp, maps, vol, vp, vp]),
        "mvs_engine_extract_mesh": (i, [vp, vol, vp, vp] + mesh_out + [pi64, pi64]),
        "mvs_engine_mesh": (i, [vp, maps, vol] + mesh_out + [pi64, pi64]),
        "mvs_default_mesh_colouring": (None, [col]),
        "mvs_engine_mesh_normals": (i, [vp] + mesh_in + [vp]),
        "mvs_engine_mesh_colours": (i, [vp, maps, col, i64, vp, vp, vp, vp]),
        "mvs_default_mesh_pruning": (None, [P(MeshPruning)]),
        "mvs_default_mesh_smoothing": (None, [P(MeshSmoothing)]),
        "mvs_engine_mesh_components": (i, [vp, i64, i64, vp, vp, vp, pi64]),
        "mvs_engine_mesh_prune": (i, [vp, P(MeshPruning)] + mesh_in + mesh_out + [vp, pi64, pi64]),
        "mvs_engine_mesh_smooth": (i, [vp, P(MeshSmoothing)] + mesh_in + [vp]),
        "mvs_default_mesh_decimation": (None, [P(MeshDecimation)]),
        "mvs_engine_mesh_decimate": (i, [vp, P(MeshDecimation)] + mesh_in + mesh_out + [vp, pi64, pi64]),
        "mvs_default_mesh_filling": (None, [P(MeshFilling)]),
        "mvs_engine_mesh_boundaries": (i, [vp, i64, i64, vp, vp, vp, pi64, pi64, pi64]),
        "mvs_engine_mesh_fill": (i, [vp, P(MeshFilling)] + mesh_in + mesh_out + [pi64, pi64, pi64]),
        "mvs_engine_mesh_render": (i, [vp] + mesh_in + [P(MeshViewRender), vp, vp, vp, vp]),
        "mvs_engine_mesh_render_lists": (i, [vp] + mesh_in + [vp]),
        "mvs_engine_mesh_visibility": (i, [vp, f] + mesh_in + [vp]),
        "mvs_engine_mesh_colours_visible": (i, [vp, maps, col, i64, vp, vp, vp, vp, vp]),
        "mvs_engine_propagate": (i, [vp, i, P(Counters)]),
        "mvs_engine_filter": (i, [vp, vp]),
        "mvs_engine_filter_stats": (i, [vp, P(FilterStats)]),
        "mvs_engine_pass": (i, [vp, i, i, P(Counters)]),
        "mvs_engine_export_counts": (i, [vp, pi64, pi64, vp]),
        "mvs_engine_export_device": (i, [vp, vp, i64, vp, i64]),
        "mvs_engine_commit_device": (i, [vp, vp, i64, vp, i64]),
        "mvs_engine_commit_local": (i, [vp]),
        "mvs_comm_unique_id": (i, [vp]),
        "mvs_engine_comm_init": (i, [vp, vp, i, i]),
        "mvs_engine_comm_attach": (i, [vp, vp, i, i]),
        "mvs_engine_comm_release": (i, [vp]),
        "mvs_engine_exchange": (i, [vp]),
        "mvs_engine_comm_info": (i, [vp, pi, pi, pi, pi]),
        "mvs_engine_depth_normal_map": (i, [vp, i, i, vp, vp, vp]),
        "mvs_engine_probe": (i, [vp, i, i64, vp, vp, vp, vp, vp]),
        "mvs_engine_last_timing": (i, [vp, P(Timing)]),
        "mvs_engine_sweep_pairs": (i, [vp, pi64]),
        "mvs_engine_sweep_repeats": (i, [vp, pi64]),
        "mvs_engine_sweep_kernels": (i, [vp, pi64]),
        "mvs_engine_sampler_launches": (i, [vp, pi64]),
    }


#: name: (restype, [argtypes]) of every entry point include/mvskit_engine.h declares, in its order
SIGNATURES = _signatures()
#: every symbol include/mvskit_engine.h declares
EXPORTS = list(SIGNATURES)


#: include/mvskit_texture.h: its struct, and its entry points in its order
TEXTURE_STRUCTS = {"mvs_mesh_texturing": MeshTexturing}


def _texture_signatures():
    P, vp, i, i64 = C.POINTER, C.c_void_p, C.c_int, C.c_int64
    tex, pi64 = P(MeshTexturing), P(C.c_int64)
    mesh_in = [i64, vp, i64, vp]               # n_v, verts, n_t, tris
    return {
        "mvs_default_mesh_texturing": (None, [tex]),
        "mvs_engine_mesh_face_views": (i, [vp, tex] + mesh_in + [vp, vp, vp, vp]),
        "mvs_engine_mesh_texture": (i, [vp, tex] + mesh_in + [vp, i64, vp, vp, pi64, pi64]),
    }


TEXTURE_SIGNATURES = _texture_signatures()


#: include/mvskit_seams.h: its struct, and its entry points in its order
SEAM_STRUCTS = {"mvs_mesh_seams": MeshSeams}


def _seam_signatures():
    P, vp, i, i64 = C.POINTER, C.c_void_p, C.c_int, C.c_int64
    seams, tex, pi64 = P(MeshSeams), P(MeshTexturing), P(C.c_int64)
    mesh_in = [i64, vp, i64, vp]               # n_v, verts, n_t, tris
    return {
        "mvs_default_mesh_seams": (None, [seams]),
        "mvs_engine_mesh_adjacency": (i, [vp, i64, i64, vp, vp, pi64]),
        "mvs_engine_mesh_face_quality": (i, [vp, tex] + mesh_in + [vp, vp]),
        "mvs_engine_mesh_smooth_labels": (i, [vp, seams, i64, i64, vp, i, vp, vp, vp, vp]),
        "mvs_engine_mesh_seam_levels": (i, [vp, seams, tex] + mesh_in + [vp, vp, vp, pi64]),
        "mvs_engine_mesh_texture_levelled": (i, [vp, tex] + mesh_in + [vp, vp, i64, vp, vp, pi64, pi64]),
    }


SEAM_SIGNATURES = _seam_signatures()


class EngineError(RuntimeError):
    """A call of the C ABI returned a negative mvs_status (`status`; include/mvskit_engine.h)."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


_libs = {}


def load_library(cap32: bool = False, cap: int = 0):
    """Loads libmvskit_engine.so (view lists of 16) -- or libmvskit_engine_cap32.so / _cap64.so, the same sources built with
    -DMVS_LISTCAP=32 / 64 (the latter with 192-byte records) -- built in-tree by mvskit_amd.build / __graft_entry__.build."""
    cap = cap or (32 if cap32 else 16)
    default = build.ENGINE_LIBS[cap]
    LIB_PATH = os.environ.get({16: "MVS_ENGINE_LIB", 32: "MVS_ENGINE_LIB32", 64: "MVS_ENGINE_LIB64"}[cap], default)  # development: A/B timing of two builds on one box
    if LIB_PATH in _libs:
        return _libs[LIB_PATH]
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"{LIB_PATH} is missing: run `python -m mvskit_amd.build` (the engine has no CPU fallback)")
    try:
        # torch bundles its own libamdhip64.so.7; two HIP runtimes in one process cannot both open the GPU.
        # Loaded first, torch's copy satisfies this library's NEEDED entry (same SONAME), so both share one.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**SIGNATURES, **TEXTURE_SIGNATURES, **SEAM_SIGNATURES}.items():
        # a build of an older revision (tools/build_variant.sh, A/B timing) lacks the newer symbols: the method that needs one raises AttributeError
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _libs[LIB_PATH] = L
    return L
