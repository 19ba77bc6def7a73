"""mvs_engine_seed_patches (DepthNormInit::createPatches' PLY branch on the device) against the code that existed before it: the host
mirror's CPU DepthNormInit::buildPatches through mvshost_seeds_from_plys on a dataset directory the test writes, uploaded with
mvs_engine_upload_patches into a second engine.  The two pools are compared as raw bytes: every record, every field, no tolerance --
both sides do the same float operations in the same order."""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

from mvskit_amd import build, engine, synth
from ply_support import GOLDEN_JPG, H, W, euler_camera, write_ply

pytestmark = pytest.mark.gpu
F = np.float32
_hosts = {}


def host_lib(cap):
    if cap not in _hosts:
        build.build_engine(cap=cap)
        engine.load_library(cap=cap)
        L = C.CDLL(build.build_host(cap=cap))
        L.mvshost_camera_probe.argtypes = [C.c_char_p, C.c_void_p]
        L.mvshost_seeds_from_plys.argtypes = [C.c_char_p, C.c_longlong, C.c_void_p]
        L.mvshost_seeds_from_plys.restype = C.c_longlong
        _hosts[cap] = L
    return _hosts[cap]


def probe_camera(host, path, text):
    path.write_text(text)
    P = np.zeros(12, F)
    assert host.mvshost_camera_probe(str(path).encode(), P.ctypes.data) == 0
    return P.reshape(3, 4)


def pixel_of(P, X):
    """PhotoSet::project at level 0 + floorf(x + 0.5f) in float32, as the mirror computes it; None behind the camera."""
    v = []
    for r in range(3):
        a = F(0)
        for k in range(3):
            a = F(a + F(P[r, k] * X[k]))
        v.append(F(a + P[r, 3]))
    if v[2] <= 0:
        return None
    return int(math.floor(F(F(v[0] / v[2]) + F(0.5)))), int(math.floor(F(F(v[1] / v[2]) + F(0.5))))


def members(ds, X, views=None):
    out = []
    for v in (range(len(ds["P"])) if views is None else views):
        if ds["masks"][v] is None:
            continue
        px = pixel_of(ds["P"][v], X)
        w, h = ds["sizes"][v]
        if px is None or not (0 <= px[0] < w and 0 <= px[1] < h) or ds["masks"][v][px[1], px[0]] <= 127:
            continue
        out.append((v, px))
    return out


def make_dataset(root, host, nv, pts, no_mask=(), near=(), holes_for=(), arc=(-15.0, 15.0), seed=5, sizes=None, intrinsics=None):
    """A dataset directory in the layout of tests/test_seed_plys.py: CONTOUR2 cameras on an arc 4 units from a plane through the origin
    (`near`: 1 unit), the 40 x 30 JPEG as every image, PGM masks with a background band and sub-threshold greys (`no_mask`: no file),
    the point cloud, one binary normal-map PLY per view with holes.  holes_for: points whose pixels carry no normal in any view.
    sizes: one (width, height) per view instead of 40 x 30 -- a binary PPM of that size as the view's image (PhotoSet::init takes
    <name>.ppm before <name>.jpg), masks and maps of that size; the cameras share the intrinsics of sizes[0], so a smaller view is a
    top-left crop.  intrinsics: one dict(fx, fy, cx, cy, skew) per view instead of the shared one.  Returns the projections the mirror derives, the level-0 masks as stored, and the maps readNormals leaves (R * n in float32)."""
    for d in ("txt", "image", "mask", "ply"):
        os.makedirs(root / d)
    (root / "option").write_text(f"level 0\ncsize 2\nthreshold 0.7\nwsize 7\nminImageNum 2\nimages -1 0 {nv}\n")
    rng = np.random.RandomState(seed)
    ds = dict(root=root, P=[], R=[], masks=[], maps=[], pts=pts.astype(F), nv=nv, sizes=[(W, H)] * nv if sizes is None else list(sizes))
    w0, h0 = ds["sizes"][0]
    intr = dict(fx=60.0 * w0 / W, fy=60.0 * w0 / W, cx=w0 / 2.0, cy=h0 / 2.0)
    for v in range(nv):
        ang = arc[0] + (arc[1] - arc[0]) * v / max(nv - 1, 1)
        th = math.radians(ang)
        dist = 1.0 if v in near else 4.0
        centre = np.array([dist * math.sin(th), 0.2 * (v % 5), -dist * math.cos(th)])
        angles = (3.0 * (v % 7) - 4.0, ang, 2.0 * (v % 3))
        _, R = euler_camera(*angles, (0.0, 0.0, 0.0))
        t = -R @ centre
        text, _ = euler_camera(*angles, t, **(intr if intrinsics is None else intrinsics[v]))
        ds["P"].append(probe_camera(host, root / "txt" / f"{v:08d}.txt", text))
        # Photo::m_R itself: with K = identity the projection the mirror derives is [R | t] exactly
        unit_k, _ = euler_camera(*angles, t, fx=1.0, fy=1.0, cx=0.0, cy=0.0)
        ds["R"].append(probe_camera(host, root / "ply" / "unit_k.txt", unit_k)[:, :3].copy())
        w, h = ds["sizes"][v]
        if sizes is None:
            shutil.copy(GOLDEN_JPG, root / "image" / f"{v:04d}0000.jpg")
        else:
            (root / "image" / f"{v:04d}0000.ppm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + rng.randint(0, 255, (h, w, 3)).astype(np.uint8).tobytes())
        if v in no_mask:
            ds["masks"].append(None)
        else:
            m = np.full((h, w), 255, np.uint8)
            m[:, : 6 + 3 * (v % 4)] = 0
            m[10:14, 20:26] = 100  # below the 127 threshold: background
            m[2:4, 30:34] = 200    # above it: foreground, though not 255
            (root / "mask" / f"{v:08d}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (w, h) + m.tobytes())
            ds["masks"].append(m)
    os.remove(root / "ply" / "unit_k.txt")
    write_ply(root / "ply" / "00000000.ply", "ascii", pts)
    hole_px = {v: set() for v in range(nv)}
    for X in holes_for:
        for v, px in members(ds, np.asarray(X, F)):
            hole_px[v].add(px)
    n_world = np.array([0.1, -0.05, -1.0])
    n_world /= np.linalg.norm(n_world)
    for v in range(nv):
        w, h = ds["sizes"][v]
        ys, xs = np.mgrid[0:h, 0:w]
        keep = (xs + 2 * ys + v) % 7 != 0  # pixels without a normal: zero vectors in the map
        for (x, y) in hole_px[v]:
            keep[y, x] = False
        xy = np.stack([xs[keep], ys[keep], np.zeros(keep.sum())], 1).astype(np.float64)
        nrm = (ds["R"][v].astype(np.float64).T @ (n_world[None] + rng.normal(0, 0.05, (len(xy), 3))).T).T
        write_ply(root / "ply" / f"{v + 1:08d}.ply", "binary_little_endian", xy, nrm, extra_colour=v % 2 == 1)
        n32, R = nrm.astype(F), ds["R"][v]
        m = np.zeros((h, w, 3), F)
        for k in range(3):  # readNormals: R[3k] * v0 + R[3k + 1] * v1 + R[3k + 2] * v2, float32, left to right
            m[ys[keep], xs[keep], k] = (R[k, 0] * n32[:, 0] + R[k, 1] * n32[:, 1]) + R[k, 2] * n32[:, 2]
        ds["maps"].append(m)
    return ds


def plane_points(n, seed=5):
    rng = np.random.RandomState(seed)
    pts = np.stack([rng.uniform(-1.4, 1.4, n), rng.uniform(-0.9, 0.9, n), 0.05 * rng.normal(size=n)], 1)
    pts[:5] += 50.0  # far outside every image
    return pts


def scene_of(ds):
    rng = np.random.RandomState(11)
    w, h = ds["sizes"][0]  # the largest view: the others are its top-left crops (Engine.set_scene(sizes=))
    base = rng.randint(0, 255, (h // 2 + 1, w // 2 + 1, 3)).astype(np.float64)
    img = np.kron(base, np.ones((2, 2, 1)))[:h, :w]
    images = np.stack([np.clip(img + 3.0 * v, 0, 255).astype(np.uint8) for v in range(ds["nv"])])
    return synth.Scene(W=w, H=h, P=np.stack(ds["P"]).astype(F), images=images, centers=np.zeros((ds["nv"], 3)))


def new_engine(ds, cap=None, **kw):
    args = dict(level=0, csize=2, wsize=7, minImageNum=2, nccThreshold=0.7, enable_check=0, seed=3)
    args.update(kw)
    e = engine.Engine(ds["nv"], list_cap=cap, **args)
    e.set_scene(scene_of(ds), sizes=ds["sizes"])
    return e


def cpu_seeds(ds, host, dtype):
    """DepthNormInit::buildPatches on the CPU: the records the parent revision uploaded."""
    out = np.zeros(len(ds["pts"]) + 8, dtype=dtype)
    n = host.mvshost_seeds_from_plys(str(ds["root"]).encode() + b"/", len(out), out.ctypes.data)
    assert 0 <= n <= len(ds["pts"]), n
    return out[:n]


def assert_same_pool(got, exp):
    assert got.dtype == exp.dtype
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        for name in got.dtype.names:
            bad = np.nonzero([not np.array_equal(a, b) for a, b in zip(np.ascontiguousarray(got[name]).view(np.uint8).reshape(len(got), -1), np.ascontiguousarray(exp[name]).view(np.uint8).reshape(len(exp), -1))])[0]
            if len(bad):
                i = bad[0]
                raise AssertionError(f"{len(bad)} of {len(got)} records differ in `{name}`, first at {i}: device {got[i]} mirror {exp[i]}")
        raise AssertionError("pools differ in padding bytes")


def device_and_mirror(ds, cap, maps=None, masks=None, **kw):
    host = host_lib(cap)
    e, o = new_engine(ds, cap, **kw), new_engine(ds, cap, **kw)
    exp = cpu_seeds(ds, host, o.dtype)
    o.upload_patches(exp)
    added = e.seed_patches(ds["pts"], ds["maps"] if maps is None else maps, ds["masks"] if masks is None else masks)
    assert added == e.num_patches() == o.num_patches()
    got, want = e.patches(), o.patches()
    assert_same_pool(got, want)
    return e, o, got, exp


def test_case1_seed_plys_layout(tmp_path):
    """4 views 40 x 30, 300 points: far-away points, mask bands and greys, map holes."""
    ds = make_dataset(tmp_path / "d", host_lib(16), 4, plane_points(300))
    e, o, got, exp = device_and_mirror(ds, 16)
    assert 100 < len(got) < 300 - 5  # points are dropped, and not only the five far ones
    assert len(set(got["nimages"].tolist())) > 1  # masks do cut view lists
    assert np.all(got["flags"] == 1) and np.all(got["nvimages"] == 0) and np.all(got["ncc"] == -1.0) and np.all(got["tmp"] == 0.0)
    # case 6, downstream: Propagate::run sees the same pool
    ce, co = e.propagate(0), o.propagate(0)
    assert ce == co and ce["patches"] > 0, (ce, co)
    assert_same_pool(e.patches(), o.patches())


def test_case2_missing_mask_null_map_behind_zero_sum_single_view(tmp_path):
    host = host_lib(16)
    behind, zero = np.array([0.1, 0.0, -2.0]), np.array([0.5, 0.2, 0.0])
    # views 1 and 3 take no part: in the dataset neither has a mask file; the device call gets view 1 without a mask and view 3 with a
    # mask but without a map.  View 4 stands 1 unit from the plane: the point at z = -2 lies behind it and in front of views 0 and 2.
    probe = make_dataset(tmp_path / "probe", host, 5, plane_points(10), no_mask=(1, 3), near=(4,))
    single = None
    for x in np.linspace(-1.4, 1.4, 281):
        X = np.array([x, 0.3, 0.0], F)
        if len(members(probe, X)) == 1:
            single = X.astype(np.float64)
            break
    assert single is not None
    pts = np.vstack([plane_points(200), behind, zero, single])
    ds = make_dataset(tmp_path / "d", host, 5, pts, no_mask=(1, 3), near=(4,), holes_for=[zero])
    assert pixel_of(ds["P"][4], behind.astype(F)) is None and len(members(ds, behind.astype(F))) >= 2
    mz = members(ds, zero.astype(F))
    assert len(mz) >= 2 and all(np.all(ds["maps"][v][py, px] == 0) for v, (px, py) in mz)
    assert len(members(ds, single.astype(F))) == 1
    maps = list(ds["maps"])
    maps[3] = None
    masks = list(ds["masks"])
    masks[3] = np.full((H, W), 255, np.uint8)
    assert masks[1] is None
    e, o, got, exp = device_and_mirror(ds, 16, maps=maps, masks=masks)
    coords = {tuple(c[:3]) for c in got["coord"].tolist()}
    key = lambda X: tuple(float(F(v)) for v in X)  # noqa: E731
    assert key(behind) in coords       # kept by the views in front of which it lies
    rec = got[[tuple(c[:3]) == key(behind) for c in got["coord"].tolist()].index(True)]
    assert 4 not in rec["images"][: rec["nimages"]].tolist()
    assert key(zero) not in coords     # summed normal exactly zero
    assert key(single) not in coords   # one view is not enough
    assert not np.any(np.isin(got["images"][:, 0], (1, 3)))
    for r in got:
        assert not set(r["images"][: r["nimages"]].tolist()) & {1, 3}


@pytest.mark.parametrize("nv,cap", [(20, 16), (40, 64)])
def test_case3_more_views_than_the_list_holds(tmp_path, nv, cap):
    ds = make_dataset(tmp_path / "d", host_lib(cap), nv, plane_points(120), arc=(-30.0, 30.0))
    e, o, got, exp = device_and_mirror(ds, cap)
    assert e.list_cap == cap and got.dtype.itemsize == (192 if cap == 64 else 128)
    if cap == 16:
        assert exp["nimages"].max() > 16 and got["nimages"].max() == 16  # the mirror's lists are cut on upload, after the sort
    else:
        assert got["nimages"].max() > 32  # nothing cut
    assert len(got) > 50


def test_case4_append_capacity_state(tmp_path):
    ds = make_dataset(tmp_path / "d", host_lib(16), 4, plane_points(300))
    host = host_lib(16)
    o = new_engine(ds, 16)
    exp = cpu_seeds(ds, host, o.dtype)
    o.upload_patches(exp)
    want = o.patches()
    n = len(want)
    # two calls append: the halves of the cloud give the whole
    e = new_engine(ds, 16)
    a = e.seed_patches(ds["pts"][:150], ds["maps"], ds["masks"])
    b = e.seed_patches(ds["pts"][150:], ds["maps"], ds["masks"])
    assert 0 < a < n and a + b == n
    assert_same_pool(e.patches(), want)
    # one record short: refused, the pool as it was
    c = new_engine(ds, 16, max_patches=n + 3 - 1)
    c.upload_patches(exp[:3])
    before = c.patches()
    with pytest.raises(engine.EngineError) as err:
        c.seed_patches(ds["pts"], ds["maps"], ds["masks"])
    assert err.value.status == -4  # MVS_ERR_CAPACITY
    assert c.num_patches() == 3
    assert_same_pool(c.patches(), before)
    # exactly enough room: accepted
    d = new_engine(ds, 16, max_patches=n + 3)
    d.upload_patches(exp[:3])
    assert d.seed_patches(ds["pts"], ds["maps"], ds["masks"]) == n
    # a pass waiting for its commit
    cnt = engine.Counters()
    assert e.L.mvs_engine_pass(e.h, 0, 0, C.byref(cnt)) == 0
    with pytest.raises(engine.EngineError) as err:
        e.seed_patches(ds["pts"], ds["maps"], ds["masks"])
    assert err.value.status == -2  # MVS_ERR_STATE
    assert e.L.mvs_engine_commit_local(e.h) == 0
    # views not set
    bare = engine.Engine(4, level=0)
    with pytest.raises(engine.EngineError) as err:
        bare.seed_patches(ds["pts"], ds["maps"], ds["masks"])
    assert err.value.status == -2


def test_case5_same_bytes_from_two_engines():
    """Several hundred thousand points: guards the order-preserving compaction (no CPU expectation here)."""
    sc = synth.make_scene(nviews=4, W=640, H=480, arc_deg=40.0, radius=4.0, kind="multi")
    valid = ~np.isnan(sc.points).any(axis=3)
    pts = np.concatenate([sc.points[v][valid[v]][v % 3::3] for v in range(sc.nviews)])
    assert len(pts) > 300000
    maps = [np.nan_to_num(sc.normals[v], nan=0.0).astype(F) for v in range(sc.nviews)]
    masks = [np.where(valid[v], 255, 0).astype(np.uint8) for v in range(sc.nviews)]
    pools = []
    for _ in range(2):
        e = engine.Engine(sc.nviews, level=0, csize=2, minImageNum=2, max_patches=len(pts))
        e.set_scene(sc)
        n = e.seed_patches(pts, maps, masks)
        assert len(pts) // 2 < n <= len(pts)
        pools.append(e.patches())
        e.close()
    assert pools[0].tobytes() == pools[1].tobytes()
    # point order is kept: the first records are a subsequence of the cloud
    coords, j = pools[0]["coord"][:, :3], 0
    for i in range(len(pts)):
        if j < len(coords) and np.array_equal(pts[i], coords[j]):
            j += 1
        if j == 2000:
            break
    assert j == min(2000, len(coords))


@pytest.mark.parametrize("sizes", [[(321, 243)] * 4, [(321, 243), (320, 243), (301, 220), (321, 236)]], ids=["odd", "unequal"])
def test_case7_odd_and_unequal_view_sizes(tmp_path, sizes):
    """Views of 321 x 243 (odd both ways: level-0 pixel tests against W and H, maps and masks with an odd row pitch), and four views
    of unequal size (every view's own W, H, map and mask in the kernel and in Engine.seed_patches' per-view shape check): records
    byte for byte against the mirror's loop.  Points near the right and bottom borders make sure the per-view bounds decide: the
    view lists of the unequal case differ from those the same points get when every view has the full size."""
    host = host_lib(16)
    rng = np.random.RandomState(9)
    edge = np.stack([rng.uniform(0.9, 1.45, 200), rng.uniform(-0.95, 0.95, 200), 0.02 * rng.normal(size=200)], 1)   # right border
    low = np.stack([rng.uniform(-1.4, 1.4, 200), rng.uniform(0.6, 1.1, 200), 0.02 * rng.normal(size=200)], 1)       # bottom border
    pts = np.vstack([plane_points(300), edge, low])
    ds = make_dataset(tmp_path / "d", host, 4, pts, sizes=sizes)
    assert [m.shape for m in ds["masks"]] == [(h, w) for w, h in sizes] and [m.shape for m in ds["maps"]] == [(h, w, 3) for w, h in sizes]
    e, o, got, exp = device_and_mirror(ds, 16)
    assert 300 < len(got) < len(pts) - 5
    lists = [tuple(r["images"][: r["nimages"]].tolist()) for r in got]
    assert len(set(lists)) > 4
    if len(set(sizes)) > 1:
        full = dict(ds, sizes=[sizes[0]] * 4, masks=[np.pad(m, ((0, sizes[0][1] - m.shape[0]), (0, sizes[0][0] - m.shape[1])), constant_values=255)
                                                    for m in ds["masks"]])
        cut = sum(len(members(full, X)) != len(members(ds, X)) for X in ds["pts"])
        assert cut > 20, cut  # points some view sees only beyond its own, smaller size
        with pytest.raises(ValueError):
            e.seed_patches(ds["pts"], [ds["maps"][0]] * 4, ds["masks"])  # view 2's map must have view 2's shape
    ce, co = e.propagate(0), o.propagate(0)
    assert ce == co, (ce, co)
    assert_same_pool(e.patches(), o.patches())


def test_case8_unequal_intrinsics(tmp_path):
    """4 views 40 x 30 whose intrinsics differ (the `intrinsics` family of tests/camera_scenes.py at this size: fx = 60 * (1, 1.25, 0.85,
    1.1), fy = 1.07 fx, skew 0.02 fx, the principal point off centre by (0, 0), (9.5, -6.25), (-12, 4), (3, 3) pixels at W = 160): the
    kernel's SeedCam table read per view, records byte for byte against the mirror's loop, and the same pool after one Propagate::run.
    The view lists differ from those the same points get when every view has the shared intrinsics of the other cases."""
    host = host_lib(16)
    intr = []
    for v in range(4):
        fx = 60.0 * (1.0, 1.25, 0.85, 1.1)[v]
        dx, dy = ((0.0, 0.0), (9.5, -6.25), (-12.0, 4.0), (3.0, 3.0))[v]
        intr.append(dict(fx=fx, fy=1.07 * fx, skew=0.02 * fx, cx=W / 2.0 + dx * W / 160.0, cy=H / 2.0 + dy * W / 160.0))
    pts = plane_points(300)
    ds = make_dataset(tmp_path / "d", host, 4, pts, intrinsics=intr)
    for v in range(4):  # the mirror derived what the family asks for: rows 0 and 1 of P differ in scale by 1.07 and by view
        K = ds["P"][v][:, :3].astype(np.float64) @ ds["R"][v].astype(np.float64).T
        np.testing.assert_allclose(K, [[intr[v]["fx"], intr[v]["skew"], intr[v]["cx"]], [0, intr[v]["fy"], intr[v]["cy"]], [0, 0, 1]], rtol=0, atol=1e-4)
    e, o, got, exp = device_and_mirror(ds, 16)
    assert 100 < len(got) < 300 - 5  # case 1's bounds: points are dropped, and not only the five far ones
    assert len(set(got["nimages"].tolist())) > 1
    shared = make_dataset(tmp_path / "s", host, 4, pts)
    moved = sum([v for v, _ in members(shared, X)] != [v for v, _ in members(ds, X)] for X in ds["pts"])
    assert moved > 20, moved
    ce, co = e.propagate(0), o.propagate(0)
    assert ce == co and ce["patches"] > 0, (ce, co)
    assert_same_pool(e.patches(), o.patches())
