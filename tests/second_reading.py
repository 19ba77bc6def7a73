"""A second reading of the reference arithmetic in numpy float32, operation by operation (image/image.cpp, image/camera.cpp,
pmmvps/optim.cpp, pmmvps/filter.cpp): what tests/test_oracle_second_reading.py holds the CPU oracle to, and what the scenes of
edge_scenes.py and the decision tests are built on.  numpy only, no GPU (a helper module like mesh_reading.py)."""
import numpy as np

F = np.float32
ASCALE = F(np.pi / F(48.0))  # Optim::refinePatch, optim.cpp:487


# ------------------------------------------------------------------ image/image.cpp
def ref_pyr_down(img):
    """Image::buildImagePyramid, image.cpp:245-315, filter 0: 4x4 [1 3 3 1]x[1 3 3 1]/64 at stride 2, taps outside the image
    dropped without renormalising, divided by mask.sum() (= 1) again, round half up."""
    H, W = img.shape[:2]
    h, w = H // 2, W // 2
    mask = np.array([[1, 3, 3, 1], [3, 9, 9, 3], [3, 9, 9, 3], [1, 3, 3, 1]], dtype=F)
    mask = (mask / mask.sum()).astype(F)
    out = np.zeros((h, w, 3), np.uint8)
    src = img.astype(F)
    for y in range(h):
        for x in range(w):
            color = np.zeros(3, F)
            for i in range(-1, 3):
                yt = 2 * y + i
                if yt < 0 or H - 1 < yt:
                    continue
                for j in range(-1, 3):
                    xt = 2 * x + j
                    if xt < 0 or W - 1 < xt:
                        continue
                    color = (color + mask[i + 1, j + 1] * src[yt, xt]).astype(F)
            color = (color / mask.sum(dtype=F)).astype(F)
            out[y, x] = np.floor(color + F(0.5)).astype(np.int32).astype(np.uint8)
    return out


def ref_get_color(img, x, y):
    """Image::getColor(float, float, level), bilinear branch, image.cpp:447-472."""
    lx, ly = int(x), int(y)
    dx1 = F(x) - F(lx)
    dx0 = F(1) - dx1
    dy1 = F(y) - F(ly)
    dy0 = F(1) - dy1
    f00, f01, f10, f11 = dx0 * dy0, dx0 * dy1, dx1 * dy0, dx1 * dy1
    p = img.astype(F)
    c = (p[ly, lx] * f00 + p[ly + 1, lx] * f01).astype(F)
    c = (c + (p[ly, lx + 1] * f10 + p[ly + 1, lx + 1] * f11).astype(F)).astype(F)
    return c


# ------------------------------------------------------------------ image/camera.cpp
def ref_project(P, X):
    """Camera::project, camera.cpp:310-326 (P = m_projections[level])."""
    ic = (P.astype(F) @ X.astype(F)).astype(F)
    if ic[2] <= 0:
        return np.array([-65535, -65535, -1], F)
    return (ic / ic[2]).astype(F)


def ref_unproject(P, ic):
    """Camera::unproject, camera.cpp:329-337."""
    M = P[:, :3].astype(np.float64)
    b = ic.astype(F) - P[:, 3].astype(F)
    return np.append((np.linalg.inv(M) @ b.astype(np.float64)).astype(F), F(1))


class RefCam:
    """Camera::updateCamera (camera.cpp:65-100) + Optim::setAxesScales (optim.cpp:43-65) for one view."""

    def __init__(self, P0, level):
        self.P = [P0.astype(F)]
        for _ in range(1, level + 3):
            q = self.P[-1].copy()
            q[:2] = (q[:2] / F(2)).astype(F)  # updateProjection, camera.cpp:91-100
            self.P.append(q)
        M = P0[:, :3].astype(np.float64)
        self.center = np.append((-np.linalg.inv(M) @ P0[:, 3].astype(np.float64)).astype(F), F(1))  # getCameraCenter, :295-308
        o = P0[2].astype(F)
        self.oaxis = (o / np.linalg.norm(o[:3]).astype(F)).astype(F)  # camera.cpp:76-80
        z = self.oaxis[:3]
        x = P0[0, :3].astype(F)
        y = np.cross(z, x).astype(F)
        y = (y / np.linalg.norm(y).astype(F)).astype(F)
        x = np.cross(y, z).astype(F)
        self.xaxis, self.yaxis, self.zaxis = x, y, z
        self.ipscale = F(np.dot(P0[0].astype(F), np.append(x, F(0)))) + F(np.dot(P0[1].astype(F), np.append(y, F(0))))


# ------------------------------------------------------------------ pmmvps/optim.cpp
def ref_get_unit(cam, coord, level):
    """Optim::getUnit, optim.cpp:34-41 (evaluated in double, returned as float)."""
    fz = np.linalg.norm((coord - cam.center).astype(F)).astype(F)
    if cam.ipscale == 0:
        return F(1)
    return F(2.0 * float(fz) * (1 << level) / float(cam.ipscale))


def ref_get_paxes(cam, coord, normal, level):
    """Optim::getPAxes, optim.cpp:67-84."""
    pscale = ref_get_unit(cam, coord, level)
    n3 = normal[:3].astype(F)
    y3 = np.cross(n3, cam.xaxis).astype(F)
    y3 = (y3 / np.linalg.norm(y3).astype(F)).astype(F)
    x3 = np.cross(y3, n3).astype(F)
    px = (np.append(x3, F(0)) * pscale).astype(F)
    py = (np.append(y3, F(0)) * pscale).astype(F)
    c0 = ref_project(cam.P[level], coord)
    xdis = np.linalg.norm((ref_project(cam.P[level], (coord + px).astype(F)) - c0).astype(F)).astype(F)
    ydis = np.linalg.norm((ref_project(cam.P[level], (coord + py).astype(F)) - c0).astype(F)).astype(F)
    return (px / xdis).astype(F), (py / ydis).astype(F)


def ref_get_tex(cam, pyr, coord, px, py, pz, level, wsize, cos_thr):
    """Optim::getTex (optim.cpp:790-844) with getTexSafe (895-915); pyr[l] = HxWx3 uint8."""
    ray = (cam.center - coord).astype(F)
    ray = (ray / np.linalg.norm(ray).astype(F)).astype(F)
    weight = max(F(0), F(np.dot(ray, pz)))
    if weight < cos_thr:
        return None
    margin = wsize // 2
    center = ref_project(cam.P[level], coord)
    dx = (ref_project(cam.P[level], (coord + px).astype(F)) - center).astype(F)
    dy = (ref_project(cam.P[level], (coord + py).astype(F)) - center).astype(F)
    ratio = (np.linalg.norm(dx).astype(F) + np.linalg.norm(dy).astype(F)) / F(2)
    ld = int(np.floor(np.log(float(ratio)) / np.log(2.0) + 0.5))
    ld = max(-level, min(2, ld))
    scale = F(2.0 ** ld)
    nl = level + ld
    center, dx, dy = (center / scale).astype(F), (dx / scale).astype(F), (dy / scale).astype(F)
    m = F(margin)
    corners = [center - dx * m - dy * m, center + dx * m - dy * m, center - dx * m + dy * m, center + dx * m + dy * m]
    xs, ys = [c[0] for c in corners], [c[1] for c in corners]
    H, W = pyr[nl].shape[:2]
    if min(xs) < 2 or W - 1 - 2 <= max(xs) or min(ys) < 2 or H - 1 - 2 <= max(ys):
        return None
    tl = (center - dx * m - dy * m).astype(F)
    tex = np.zeros((wsize * wsize, 3), F)
    for y in range(wsize):
        for x in range(wsize):
            samp = (tl + dx * F(x) + dy * F(y)).astype(F)
            tex[y * wsize + x] = ref_get_color(pyr[nl], samp[0], samp[1])
    return tex


def ref_normalize(tex):
    """Optim::normalize, optim.cpp:917-940 (sequential float sums)."""
    sz = tex.shape[0]
    ave = np.zeros(3, F)
    for t in tex:
        ave = (ave + t).astype(F)
    ave = (ave / F(sz)).astype(F)
    ssd = F(0)
    for t in tex:
        d = (t - ave).astype(F)
        ssd = F(ssd + F(np.dot(d, d)))
    msd = F(np.sqrt(ssd / F(3 * sz)))
    if msd == 0:
        msd = F(1)
    return ((tex - ave).astype(F) / msd).astype(F)


def ref_dot(t0, t1):
    """Optim::dot, optim.cpp:601-609."""
    s = F(0)
    for a, b in zip(t0, t1):
        s = F(s + F(np.dot(a, b)))
    return F(s / F(3 * t0.shape[0]))


def ref_robustincc(x):  # optim.cpp:622-624
    return F(x) / (F(1) + F(3) * F(x))


def ref_compute_incc(cams, pyrs, coord, normal, idx, level, wsize, tau, robust, cos_thr):
    """Optim::computeINCC (optim.cpp:630-706, non-PAIRNCC branch) with computeWeights (942-948) / computeUnits (109-132)."""
    if len(idx) < 2:
        return F(2)
    units = []
    for v in idx:
        u = ref_get_unit(cams[v], coord, level)
        ray = (cams[v].center - coord).astype(F)
        ray = (ray / np.linalg.norm(ray).astype(F)).astype(F)
        d = F(np.dot(ray, normal))
        units.append(F(u / d) if d > 0 else F(2 ** 31 // 2))
    w = [F(1)] + [min(F(1), F(units[0] / u)) for u in units[1:]]
    px, py = ref_get_paxes(cams[idx[0]], coord, normal, level)
    sz = min(tau, len(idx))
    texs = []
    for i in range(sz):
        t = ref_get_tex(cams[idx[i]], pyrs[idx[i]], coord, px, py, normal, level, wsize, cos_thr)
        texs.append(None if t is None else ref_normalize(t))
    if texs[0] is None:
        return F(2)
    score, total = F(0), F(0)
    for i in range(1, sz):
        if texs[i] is None:
            continue
        total = F(total + w[i])
        incc = F(1.0 - float(ref_dot(texs[0], texs[i])))
        score = F(score + (ref_robustincc(incc) if robust else incc) * w[i])
    return F(2) if total == 0 else F(score / total)


def ref_mask_down(mask):
    """Image::buildMaskPyramid, image.cpp:717-747: a pixel of the next level is 255 if any of the four pixels (2x, 2x + 1) x (2y, 2y + 1)
    of the level above is set.  The reference bounds 2x + 1 by the width itself, not by width - 1; with w = W / 2 rounded down
    2x + 1 <= W - 1 for every x < w, so the bound never acts and an odd parent's last column and row are never read."""
    H, W = mask.shape
    h, w = H // 2, W // 2
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        ys = (2 * y, min(H, 2 * y + 1))
        for x in range(w):
            xs = (2 * x, min(W, 2 * x + 1))
            inside = sum(1 for j in range(2) for i in range(2) if mask[ys[j], xs[i]])
            out[y, x] = 255 if inside > 0 else 0
    return out


def ref_get_mask_all(cams, masks, X, level):
    """PhotoSet::getMask(coord, level), photoSet.cpp:223-233, over Image::getMask, image.cpp:749-781: 0 if the point projects onto
    a zero mask pixel of any view, else -1 (a projection outside a view's image does not count against it)."""
    for cam, m in zip(cams, masks):
        ic = ref_project(cam.P[level], X)
        ix, iy = int(np.floor(ic[0] + F(0.5))), int(np.floor(ic[1] + F(0.5)))
        H, W = m[level].shape
        if ix < 0 or W <= ix or iy < 0 or H <= iy:
            continue
        if m[level][iy, ix] == 0:
            return 0
    return -1


# ------------------------------------------------------------------ refinement variables, cost, scales, neighbours
def ref_encode(cam, center, ray, dscale, coord, normal):
    """Optim::encode, optim.cpp:549-580 (libm calls; the oracle's own polynomials are within 3e-7 of them)."""
    x0 = F(np.dot((coord - center).astype(F), ray)) / F(dscale)
    n3 = normal[:3].astype(F)
    fx, fy, fz = F(np.dot(cam.xaxis, n3)), F(np.dot(cam.yaxis, n3)), F(np.dot(cam.zaxis, n3))
    a2 = F(np.arcsin(max(F(-1), min(F(1), fy))))
    cosb = F(np.cos(a2))
    if cosb == 0:
        a1 = F(0)
    else:
        sina, cosa = F(fx / cosb), F(-fz / cosb)
        a1 = F(np.arccos(max(F(-1), min(F(1), cosa))))
        if sina < 0:
            a1 = -a1
    return np.array([x0, a1 / ASCALE, a2 / ASCALE], F)


def ref_decode(cam, center, ray, dscale, x):
    """Optim::decode, optim.cpp:582-599."""
    coord = (center + F(dscale) * F(x[0]) * ray).astype(F)
    a1, a2 = F(x[1] * ASCALE), F(x[2] * ASCALE)
    fx, fy, fz = F(np.sin(a1) * np.cos(a2)), F(np.sin(a2)), F(-np.cos(a1) * np.cos(a2))
    n3 = (cam.xaxis * fx + cam.yaxis * fy + cam.zaxis * fz).astype(F)
    return coord, np.append(n3, F(0))


def ref_cost_func(cams, pyrs, center, ray, dscale, idx, x, level, wsize, tau, min_image_num, cos_thr):
    """Optim::cost_func, optim.cpp:401-468 (the non-pairwise branch)."""
    coord, normal = ref_decode(cams[idx[0]], center, ray, dscale, x)
    px, py = ref_get_paxes(cams[idx[0]], coord, normal, level)
    sz = min(tau, len(idx))
    minimum = min(min_image_num, sz)
    texs = []
    for i in range(sz):
        t = ref_get_tex(cams[idx[i]], pyrs[idx[i]], coord, px, py, normal, level, wsize, cos_thr)
        texs.append(None if t is None else ref_normalize(t))
    if texs[0] is None:
        return 2.0
    ans, denom = 0.0, 0
    for i in range(1, sz):
        if texs[i] is None:
            continue
        ans += float(ref_robustincc(F(1.0 - float(ref_dot(texs[0], texs[i])))))
        denom += 1
    return 2.0 if denom < minimum - 1 else ans / denom


def ref_set_scales(cams, coord, idx, level, wsize, tau):
    """PatchManager::setScales, patch_manager.cpp:378-399 (m_dscale starts at 0, patch.cpp:13-25)."""
    unit = ref_get_unit(cams[idx[0]], coord, level)
    unit2 = F(2) * unit
    ray = (coord - cams[idx[0]].center).astype(F)
    ray = (ray / np.linalg.norm(ray).astype(F)).astype(F)
    num = min(tau, len(idx))
    ds = F(0)
    for i in range(1, num):
        P = cams[idx[i]].P[level]
        diff = (ref_project(P, coord) - ref_project(P, (coord - unit2 * ray).astype(F))).astype(F)
        ds = F(ds + np.linalg.norm(diff).astype(F))
    ds = F(ds / F(num - 1))
    ds = F(unit2 / ds)
    return ds, F(np.arctan(ds / (unit * F(wsize) / F(2))))


def ref_is_neighbor(cams, a, b, csize, level, thr):
    """PmMvps::isNeighbor, pmmvps.cpp:117-147 -- including the reference's constant cosf(120 / pi * 180)."""
    hunit = F((ref_get_unit(cams[int(a["images"][0])], a["coord"].astype(F), level) + ref_get_unit(cams[int(b["images"][0])], b["coord"].astype(F), level)) / F(2) * F(csize))
    na, nb = a["normal"].astype(F), b["normal"].astype(F)
    if F(np.dot(na, nb)) < F(np.cos(F(F(120.0) / F(np.pi) * F(180.0)))):
        return 0
    diff = (a["coord"] - b["coord"]).astype(F)
    vunit = F(a["dscale"] + b["dscale"])
    f0, f1 = F(np.dot(na, diff)), F(np.dot(nb, diff))
    ftmp = F(F(abs(f0) + abs(f1)) / F(2) / vunit)
    hsize = F(np.linalg.norm((diff - f0 * na + diff - f1 * nb).astype(F)).astype(F) / F(2) / hunit)
    if 1.0 < hsize:
        ftmp = F(ftmp / min(F(2), hsize))
    return 1 if ftmp < thr else 0


def ref_quad_residual(cams, rec, coords, level, tau):
    """Filter::filterQuad / ortho / lls, filter.cpp:329-430: the least-squares quadric through the neighbours by SVD
    (Eigen's jacobiSvd().solve there, numpy's lstsq here), in float like the reference."""
    z = rec["normal"].astype(F)
    if abs(z[0]) > 0.5:
        x = np.array([z[1], -z[0], 0, 0], F)
    elif abs(z[1]) > 0.5:
        x = np.array([0, z[2], -z[1], 0], F)
    else:
        x = np.array([-z[2], 0, z[0], 0], F)
    x = (x / np.linalg.norm(x).astype(F)).astype(F)
    y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0], 0], F)
    diff = (coords.astype(F) - rec["coord"].astype(F)).astype(F)
    h = F(0)
    for d in diff:
        h = F(h + np.linalg.norm(d).astype(F))
    h = F(h / F(len(diff)))
    fx, fy, fz = (diff @ x / h).astype(F), (diff @ y / h).astype(F), (diff @ z).astype(F)
    A = np.stack([fx * fx, fy * fy, fx * fy, fx, fy], 1).astype(F)
    sol = np.linalg.lstsq(A, fz, rcond=None)[0].astype(F)
    idx = [int(i) for i in rec["images"][: rec["nimages"]]]
    inum = min(tau, len(idx))
    unit = F(0)
    for i in range(inum):
        unit = F(unit + ref_get_unit(cams[idx[i]], rec["coord"].astype(F), level))
    unit = F(unit / F(inum))
    res = F(0)
    for n in range(len(diff)):
        r = sol[0] * (fx[n] * fx[n]) + sol[1] * (fy[n] * fy[n]) + sol[2] * (fx[n] * fy[n]) + sol[3] * fx[n] + sol[4] * fy[n] - fz[n]
        res = F(res + F(abs(r)) / unit)
    return F(res / F(len(diff) - 5))
