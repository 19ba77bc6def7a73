"""Which C calls the size-then-fill methods of engine.Engine make, in which order and with which arguments: checked against a stand-in
library that records every call, writes chosen counts through the byref arguments and returns a chosen status.  No library, no GPU."""
import ctypes as C

import numpy as np
import pytest

from mvskit_amd import engine

HANDLE = 0x1234
REF, PTR = "ref", "ptr"  # a byref(c_int64) count; a non-null c_void_p


def _seen(a):
    """an argument as the assertions below spell it"""
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, C.c_void_p):
        return "h" if a.value == HANDLE else PTR
    if isinstance(a, C.Array):
        return f"{a._type_.__name__}[{len(a)}]"
    obj = getattr(a, "_obj", None)  # byref(...)
    if isinstance(obj, C.c_int64):
        return REF
    if isinstance(obj, C.Structure):
        return type(obj).__name__
    raise AssertionError(f"unexpected argument {a!r}")


class StandIn:
    """script: one (status, counts) per call, in call order; counts go to the call's byref(c_int64) arguments, in their order"""

    def __init__(self, script):
        self.script, self.calls = list(script), []

    def __getattr__(self, name):
        if name == "mvs_last_error":
            return lambda: b"stand-in"

        def fn(*args):
            self.calls.append((name, tuple(_seen(a) for a in args)))
            if name.startswith("mvs_default_"):
                return None
            status, counts = self.script.pop(0)
            refs = [a._obj for a in args if isinstance(getattr(a, "_obj", None), C.c_int64)]
            assert len(refs) == len(counts), (name, counts)
            for r, v in zip(refs, counts):
                r.value = v
            return status

        return fn


def make(script):
    e = engine.Engine.__new__(engine.Engine)
    e.L, e.h, e.cfg = StandIn(script), C.c_void_p(HANDLE), engine.Config()
    return e


def done(e):
    """the calls made, with the script used up; the handle is dropped so that nothing is recorded behind the test"""
    e.h = None
    assert e.L.script == []
    return e.L.calls


VOLUME = engine.make_volume((0, 0, 0), 1.0, (2, 2, 2), 4.0)
TSDF = np.zeros(8, np.float32)
VERTS = np.arange(12, dtype=np.float32).reshape(4, 3)
TRIS = np.array([[0, 1, 2], [1, 2, 3]], np.int32)


def check_mesh(verts, tris, n_v, n_t):
    assert verts.shape == (n_v, 3) and verts.dtype == np.float32 and verts.flags.owndata
    assert tris.shape == (n_t, 3) and tris.dtype == np.int32 and tris.flags.owndata


# ---- _mesh without caps (extract_mesh; mesh() with no or half an estimate)
@pytest.mark.parametrize("n_v, n_t", [(5, 7), (3, 0), (0, 2)])
def test_size_call_then_full_call_with_the_reported_counts(n_v, n_t):
    e = make([(0, (n_v, n_t)), (0, (n_v, n_t))])
    verts, tris = e.extract_mesh(VOLUME, TSDF)
    check_mesh(verts, tris, n_v, n_t)
    head = ("h", "Volume", PTR, None)
    assert done(e) == [("mvs_engine_extract_mesh", head + (0, None, 0, None, REF, REF)),
                       ("mvs_engine_extract_mesh", head + (n_v, PTR, n_t, PTR, REF, REF))]


def test_empty_result_takes_the_size_call_only():
    e = make([(0, (0, 0))])
    verts, tris = e.extract_mesh(VOLUME, TSDF, count=np.ones(8, np.int32))
    check_mesh(verts, tris, 0, 0)
    assert done(e) == [("mvs_engine_extract_mesh", ("h", "Volume", PTR, PTR, 0, None, 0, None, REF, REF))]


@pytest.mark.parametrize("caps", [{}, {"cap_v": 10}, {"cap_t": 10}])
def test_mesh_without_both_caps_makes_the_size_call_first(caps):
    e = make([(0, (5, 7)), (0, (5, 7))])
    check_mesh(*e.mesh(VOLUME, **caps), 5, 7)
    head = ("h", "MapsConfig", "Volume")
    assert done(e) == [("mvs_default_maps_config", ("MapsConfig",)), ("mvs_engine_mesh", head + (0, None, 0, None, REF, REF)),
                       ("mvs_engine_mesh", head + (5, PTR, 7, PTR, REF, REF))]


def test_size_call_that_fails_raises():
    e = make([(engine.MVS_ERR_STATE, (0, 0))])
    with pytest.raises(engine.EngineError) as err:
        e.mesh(VOLUME)
    assert err.value.status == engine.MVS_ERR_STATE and len(done(e)) == 2


# ---- mesh() with caps
def test_mesh_with_caps_that_fit_is_one_call():
    e = make([(0, (3, 4))])
    check_mesh(*e.mesh(VOLUME, cap_v=10, cap_t=12), 3, 4)
    assert done(e) == [("mvs_default_maps_config", ("MapsConfig",)), ("mvs_engine_mesh", ("h", "MapsConfig", "Volume", 10, PTR, 12, PTR, REF, REF))]


def test_mesh_with_caps_too_small_calls_again_with_the_reported_counts():
    e = make([(engine.MVS_ERR_CAPACITY, (20, 30)), (0, (20, 30))])
    check_mesh(*e.mesh(VOLUME, cap_v=10, cap_t=12), 20, 30)
    head = ("h", "MapsConfig", "Volume")
    assert done(e)[1:] == [("mvs_engine_mesh", head + (10, PTR, 12, PTR, REF, REF)), ("mvs_engine_mesh", head + (20, PTR, 30, PTR, REF, REF))]


@pytest.mark.parametrize("status", [engine.MVS_ERR_ARG, engine.MVS_ERR_STATE, engine.MVS_ERR_HIP, engine.MVS_ERR_NO_DEVICE])
def test_mesh_with_caps_raises_on_any_other_status(status):
    e = make([(status, (0, 0))])
    with pytest.raises(engine.EngineError) as err:
        e.mesh(VOLUME, cap_v=10, cap_t=12)
    assert err.value.status == status and "stand-in" in str(err.value)
    assert [name for name, _ in done(e)] == ["mvs_default_maps_config", "mvs_engine_mesh"]


def test_mesh_retry_that_fails_raises():
    e = make([(engine.MVS_ERR_CAPACITY, (20, 30)), (engine.MVS_ERR_HIP, (20, 30))])
    with pytest.raises(engine.EngineError) as err:
        e.mesh(VOLUME, cap_v=10, cap_t=12)
    assert err.value.status == engine.MVS_ERR_HIP and len(done(e)) == 3


# ---- prune_mesh, decimate_mesh: always two calls, vmap only on the second
@pytest.mark.parametrize("n_v, n_t", [(3, 1), (0, 0)])
@pytest.mark.parametrize("method, symbol, struct, args", [("prune_mesh", "mvs_engine_mesh_prune", "MeshPruning", (2,)),
                                                          ("decimate_mesh", "mvs_engine_mesh_decimate", "MeshDecimation", (0.5,))])
def test_prune_and_decimate_make_two_calls_with_vmap_on_the_second(method, symbol, struct, args, n_v, n_t):
    e = make([(0, (n_v, n_t)), (0, (n_v, n_t))])
    verts, tris, vmap = getattr(e, method)(VERTS, TRIS, *args)
    check_mesh(verts, tris, n_v, n_t)
    assert vmap.shape == (4,) and vmap.dtype == np.int32 and (vmap == -1).all()  # preset: the stand-in writes nothing
    head = ("h", struct, 4, PTR, 2, PTR)
    assert done(e) == [(symbol, head + (0, None, 0, None, None, REF, REF)), (symbol, head + (n_v, PTR, n_t, PTR, PTR, REF, REF))]


@pytest.mark.parametrize("method, args", [("prune_mesh", (2,)), ("decimate_mesh", (0.5,))])
def test_prune_and_decimate_raise_on_a_failed_size_call(method, args):
    e = make([(engine.MVS_ERR_ARG, (0, 0))])
    with pytest.raises(engine.EngineError) as err:
        getattr(e, method)(VERTS, TRIS, *args)
    assert err.value.status == engine.MVS_ERR_ARG and len(done(e)) == 1


# ---- fill_holes: the second call only when something is reported
def test_fill_holes_makes_the_second_call_when_something_is_reported():
    e = make([(0, (6, 8, 2)), (0, (6, 8, 2))])
    verts, tris, n_filled = e.fill_holes(VERTS, TRIS, max_edges=16)
    check_mesh(verts, tris, 6, 8)
    assert n_filled == 2 and isinstance(n_filled, int)
    head = ("h", "MeshFilling", 4, PTR, 2, PTR)
    assert done(e) == [("mvs_engine_mesh_fill", head + (0, None, 0, None, REF, REF, REF)), ("mvs_engine_mesh_fill", head + (6, PTR, 8, PTR, REF, REF, REF))]


def test_fill_holes_of_an_empty_result_takes_the_size_call_only():
    e = make([(0, (0, 0, 0))])
    verts, tris, n_filled = e.fill_holes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    check_mesh(verts, tris, 0, 0)
    assert n_filled == 0
    assert done(e) == [("mvs_engine_mesh_fill", ("h", "MeshFilling", 0, PTR, 0, PTR, 0, None, 0, None, REF, REF, REF))]


# ---- the records that become dictionaries
def test_record_dictionaries_keep_their_keys_and_value_types():
    e = make([(0, ())] * 6)
    t, f = e.timing(), e.filter_stats()
    assert set(t) == {"index_ms", "sweep_ms", "commit_ms", "sweep_launches", "exchange_ms", "exchange_bytes", "check_retried_cells", "sweep_jobs_listed"}
    assert {k for k, v in t.items() if type(v) is float} == {"index_ms", "sweep_ms", "commit_ms", "exchange_ms"}
    assert all(type(v) in (int, float) for v in t.values())
    assert list(f) == [n for n, _ in engine.FilterStats._fields_]
    assert all(type(f[k]) is (float if k.endswith("_ms") else int) for k in f)
    for method, keys in (("sweep_pairs", engine.Engine.SWEEP_PAIR_KEYS), ("sweep_repeats", engine.Engine.SWEEP_REPEAT_KEYS),
                         ("sweep_kernels", engine.Engine.SWEEP_KERNEL_KEYS), ("sampler_launches", engine.Engine.SAMPLER_LAUNCH_KEYS)):
        d = getattr(e, method)()
        assert tuple(d) == keys and all(type(v) is int for v in d.values())
    assert [name for name, _ in done(e)] == ["mvs_engine_last_timing", "mvs_engine_filter_stats", "mvs_engine_sweep_pairs", "mvs_engine_sweep_repeats",
                                             "mvs_engine_sweep_kernels", "mvs_engine_sampler_launches"]
