"""Yardsticks of the mesh rasteriser (``mofa_raster_*``).

* :func:`rasterize` restates the kernels' arithmetic in NumPy: the fp32 steps as separately rounded ``np.float32`` operations, coverage in
  ``np.int64``, interpolation in ``np.float64`` rounded once — the GPU frame must equal it bit for bit.  ``fault`` injects one mistake
  (``FAULTS``) so that tests/test_raster_reference_cpu.py can show that the checks below catch it.
* :func:`raycast` is an independent fp64 ray caster (Moller-Trumbore) on rays in the convention of ``get_rays``: nearest hit, depth as the
  ray parameter.  It shares no step with the rasteriser.
* :func:`agreement` holds one against the other: differing mask and face pixels, and the restatement's depth against the fp64 range of its
  own face's plane over the window ``(i +- 1/256, j +- 1/256)``.
* the scene builders the tests share."""
import numpy as np

from mofanerf_amd.rays import pose_spherical
from rays_reference import pose_spherical as generic_pose

f32 = np.float32
INT32_MAX = 2 ** 31 - 1
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD_BAND = f32(2 ** 20)
FAULTS = ("affine", "half_pixel", "v_flip", "swap_c", "strict", "tie_high", "no_znear")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def intrinsics(K):
    K = np.asarray(K, np.float64)
    return f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])


def pose34(c2w):
    return np.ascontiguousarray(np.asarray(c2w.detach().cpu() if hasattr(c2w, "detach") else c2w, dtype=np.float32)[:3, :4])


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def project(verts, K, c2w, znear, fault=None):
    """(X, Y int64 [V], zc float32 [V], valid bool [V]) as ``mofa_raster_project`` forms them."""
    v, c = np.asarray(verts, f32).reshape(-1, 3), pose34(c2w)
    fx, fy, cx, cy = intrinsics(K)
    if fault == "swap_c":
        cx, cy = cy, cx
    with np.errstate(all="ignore"):
        d = [v[:, a] - c[a, 3] for a in range(3)]
        p = [((d[0] * c[0, a]).astype(f32) + (d[1] * c[1, a]).astype(f32)).astype(f32) + (d[2] * c[2, a]).astype(f32) for a in range(3)]
        zc = -p[2]
        u = cx + fx * (p[0] / zc)
        w = (cy + fy * (p[1] / zc)) if fault == "v_flip" else (cy - fy * (p[1] / zc))
        valid = (np.abs(u) <= GUARD_BAND) & (np.abs(w) <= GUARD_BAND)
        if fault != "no_znear":
            valid &= zc >= f32(znear)
        X = np.where(valid, np.rint(u * f32(256)), 0).astype(np.int64)
        Y = np.where(valid, np.rint(w * f32(256)), 0).astype(np.int64)
    assert all(a.dtype == f32 for a in (zc, u, w))
    return X, Y, zc.astype(f32), valid


def _weights(Xs, Ys, s, Px, Py):
    return [s * ((Xs[q] - Xs[p]) * (Py - Ys[p]) - (Ys[q] - Ys[p]) * (Px - Xs[p])) for p, q in ((1, 2), (2, 0), (0, 1))]


def _interp(w, area, z):
    """fp64: (depth float32, b0, b1, b2)."""
    with np.errstate(all="ignore"):
        r = [(w[k].astype(np.float64) / np.float64(area)) / np.float64(z[k]) for k in range(3)]
        q = (r[0] + r[1]) + r[2]
        return (1.0 / q).astype(f32), [r[k] / q for k in range(3)]


def ray_dirs(H, W, K, c2w):
    """float32 [H,W,3]: ``pinhole_ray``'s direction per pixel, operation for operation."""
    fx, fy, cx, cy = intrinsics(K)
    c = pose34(c2w)
    i, j = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32), indexing="xy")
    d0, d1, d2 = (i - cx) / fx, -((j - cy) / fy), f32(-1)
    return np.stack([((d0 * c[a, 0]).astype(f32) + (d1 * c[a, 1]).astype(f32)).astype(f32) + f32(d2 * c[a, 2]) for a in range(3)], -1).astype(f32)


def flat_normal(v0, v1, v2):
    """(v1 - v0) x (v2 - v0) normalised, in the operation order of ``k_point_normals``; (0,0,0) unless its length is > 0."""
    du, dv = (v1 - v0).astype(f32), (v2 - v0).astype(f32)
    with np.errstate(all="ignore"):
        nx = f32(f32(du[1] * dv[2]) - f32(du[2] * dv[1]))
        ny = f32(f32(du[2] * dv[0]) - f32(du[0] * dv[2]))
        nz = f32(f32(du[0] * dv[1]) - f32(du[1] * dv[0]))
        length = np.sqrt(f32(f32(f32(nx * nx) + f32(ny * ny)) + f32(nz * nz)))
        if not length > 0:
            return np.zeros(3, f32)
        return np.array([f32(nx / length), f32(ny / length), f32(nz / length)], f32)


def rasterize(verts, faces, H, W, K, c2w, attrs=None, znear=1e-3, wave_min_pixels=INT32_MAX, fault=None):
    """dict: ``depth`` float32 [H,W], ``face`` int32 [H,W], ``bary`` float32 [H,W,3], ``normal`` float32 [H,W,3], ``attr`` float32 [H,W,C]
    (with ``attrs`` [V,C]) and ``counts`` int64 [4] = drawn, culled, degenerate, wave_path."""
    assert fault is None or fault in FAULTS
    verts, faces = np.asarray(verts, f32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(verts)
    X, Y, zc, valid = project(verts, K, c2w, znear, fault)
    off = 128 if fault == "half_pixel" else 0
    zbuf = np.full((H, W), EMPTY, np.uint64)
    counts = np.zeros(4, np.int64)
    setups = {}
    for f, tri in enumerate(faces.astype(np.int64)):
        if (tri < 0).any() or (tri >= V).any() or not valid[tri].all():
            counts[1] += 1
            continue
        Xs, Ys, zs = X[tri], Y[tri], zc[tri]
        A = (Xs[1] - Xs[0]) * (Ys[2] - Ys[0]) - (Ys[1] - Ys[0]) * (Xs[2] - Xs[0])
        if A == 0:
            counts[2] += 1
            continue
        counts[0] += 1
        s = np.int64(1 if A > 0 else -1)
        i0, i1 = max(-(-int(Xs.min()) // 256), 0), min(int(Xs.max()) // 256, W - 1)
        j0, j1 = max(-(-int(Ys.min()) // 256), 0), min(int(Ys.max()) // 256, H - 1)
        npix = (i1 - i0 + 1) * (j1 - j0 + 1) if (i1 >= i0 and j1 >= j0) else 0
        if wave_min_pixels != INT32_MAX and npix >= wave_min_pixels:
            counts[3] += 1
        setups[f] = (Xs, Ys, zs, s, abs(int(A)))
        if npix == 0:
            continue
        Px, Py = np.meshgrid(np.arange(i0, i1 + 1, dtype=np.int64) * 256 + off, np.arange(j0, j1 + 1, dtype=np.int64) * 256 + off, indexing="xy")
        w = _weights(Xs, Ys, s, Px, Py)
        cov = ((w[0] > 0) & (w[1] > 0) & (w[2] > 0)) if fault == "strict" else ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0))
        if not cov.any():
            continue
        depth, b = _interp(w, abs(int(A)), zs)
        if fault == "affine":
            l = [w[k].astype(np.float64) / np.float64(abs(int(A))) for k in range(3)]
            depth = ((l[0] * np.float64(zs[0]) + l[1] * np.float64(zs[1])) + l[2] * np.float64(zs[2])).astype(f32)
        low = np.uint64(INT32_MAX - f if fault == "tie_high" else f)
        key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
        box = zbuf[j0:j1 + 1, i0:i1 + 1]
        np.minimum(box, np.where(cov, key, EMPTY), out=box)
    hit = zbuf != EMPTY
    low = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    face = np.where(hit, (INT32_MAX - low) if fault == "tie_high" else low, -1).astype(np.int32)
    out = {"depth": np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32), "face": face,
           "bary": np.zeros((H, W, 3), f32), "normal": np.zeros((H, W, 3), f32), "counts": counts}
    if attrs is not None:
        attrs = np.asarray(attrs, f32)
        attrs = attrs.reshape(V, attrs.shape[-1])
        out["attr"] = np.zeros((H, W, attrs.shape[1]), f32)
    D = ray_dirs(H, W, K, c2w)
    for f in np.unique(face[hit]):
        Xs, Ys, zs, s, area = setups[int(f)]
        jj, ii = np.nonzero(face == f)
        w = _weights(Xs, Ys, s, ii.astype(np.int64) * 256 + off, jj.astype(np.int64) * 256 + off)
        _, b = _interp(w, area, zs)
        out["bary"][jj, ii] = np.stack(b, -1).astype(f32)
        tri = faces[f].astype(np.int64)
        if attrs is not None:
            a = attrs[tri].astype(np.float64)
            out["attr"][jj, ii] = ((b[0][:, None] * a[0] + b[1][:, None] * a[1]) + b[2][:, None] * a[2]).astype(f32)
        n = flat_normal(*verts[tri])
        d = D[jj, ii]
        sgn = ((n[0] * d[:, 0]).astype(f32) + (n[1] * d[:, 1]).astype(f32)).astype(f32) + (n[2] * d[:, 2]).astype(f32)
        out["normal"][jj, ii] = np.where((sgn > 0)[:, None], -n, n)
    return out


# ---- the independent ray caster --------------------------------------------------------------------------------------------------------
def camera64(K, c2w):
    K = np.asarray(K, np.float64)
    c = pose34(c2w).astype(np.float64)
    return (float(f32(K[0, 0])), float(f32(K[1, 1])), float(f32(K[0, 2])), float(f32(K[1, 2]))), c[:, :3], c[:, 3]


def rays64(x, y, K, c2w):
    """fp64 ray directions through the image points (x, y) (any shape), as ``get_rays`` defines them: R [(x-cx)/fx, -(y-cy)/fy, -1]."""
    (fx, fy, cx, cy), R, _ = camera64(K, c2w)
    cam = np.stack([(x - cx) / fx, -(y - cy) / fy, -np.ones_like(x)], -1)
    return cam @ R.T


def raycast(verts, faces, H, W, K, c2w):
    """(depth float64 [H,W] (0 where nothing is hit), face int32 [H,W] (-1)): nearest two-sided Moller-Trumbore hit with t > 0; the lower
    face index among equal t."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    _, _, o = camera64(K, c2w)
    ok = ((faces >= 0) & (faces < len(verts))).all(-1) & np.isfinite(verts[np.clip(faces, 0, max(len(verts) - 1, 0))]).all((-1, -2)) if len(verts) else np.zeros(len(faces), bool)
    ids = np.flatnonzero(ok)
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = rays64(i, j, K, c2w).reshape(-1, 1, 3)                                      # [P,1,3]
    best_t, best_f = np.full(H * W, np.inf), np.full(H * W, -1, np.int64)
    for lo in range(0, len(ids), 512):
        tri = verts[faces[ids[lo:lo + 512]]]                                        # [F,3,3]
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        pv = np.cross(d, e2[None])                                                  # [P,F,3]
        det = (pv * e1[None]).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = (o - tri[:, 0])[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (qv * d).sum(-1) * inv
            t = (qv * e2[None]).sum(-1) * inv
            good = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        t = np.where(good, t, np.inf)
        k = t.argmin(-1)
        tk = t[np.arange(len(t)), k]
        better = tk < best_t
        best_t[better], best_f[better] = tk[better], ids[lo:lo + 512][k[better]]
    hit = np.isfinite(best_t)
    return np.where(hit, best_t, 0.0).reshape(H, W), np.where(hit, best_f, -1).astype(np.int32).reshape(H, W)


def plane_depth_window(verts, faces, face_map, K, c2w, half=1.0 / 256):
    """(lo, hi) float64 [H,W]: the range of the depth (ray parameter) of each covered pixel's OWN face's plane over the window
    (i +- half, j +- half), from the unsnapped fp64 vertices.  1/depth is affine on the screen, so the range is spanned by the corners."""
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    _, _, o = camera64(K, c2w)
    H, W = face_map.shape
    lo, hi = np.zeros((H, W)), np.zeros((H, W))
    jj, ii = np.nonzero(face_map >= 0)
    tri = verts[faces[face_map[jj, ii]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    num = (n * (tri[:, 0] - o)).sum(-1)
    ts = []
    for dx in (-half, half):
        for dy in (-half, half):
            d = rays64(ii + dx, jj + dy, K, c2w)
            with np.errstate(all="ignore"):
                ts.append(num / (n * d).sum(-1))
    ts = np.stack(ts, -1)
    lo[jj, ii], hi[jj, ii] = ts.min(-1), ts.max(-1)
    return lo, hi


WINDOW_WIDEN = 2.0 ** -22
DISAGREE_CAP = 0.02


def agreement(rast, cast, verts, faces, K, c2w):
    """Hold a rasterised frame (dict of :func:`rasterize`, or of the GPU) against the ray caster's ``(depth, face)``:
    ``covered`` (pixels the rasteriser covers), ``mask_diff``, ``face_diff`` (covered by both, another face), ``outside`` (covered pixels
    whose depth leaves the window of :func:`plane_depth_window` widened by 2^-22 relative) and ``disagree`` = (mask_diff + face_diff) / covered."""
    face, depth = np.asarray(rast["face"]), np.asarray(rast["depth"], np.float64)
    m_r, m_c = face >= 0, cast[1] >= 0
    lo, hi = plane_depth_window(verts, faces, face, K, c2w)
    inside = (depth >= lo * (1 - WINDOW_WIDEN)) & (depth <= hi * (1 + WINDOW_WIDEN))
    covered = int(m_r.sum())
    out = {"covered": covered, "mask_diff": int((m_r != m_c).sum()), "face_diff": int((m_r & m_c & (face != cast[1])).sum()),
           "outside": int((m_r & ~inside).sum())}
    out["disagree"] = (out["mask_diff"] + out["face_diff"]) / max(covered, 1)
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def uv_sphere(stacks, slices, radius=1.0, centre=(0.1, -0.05, 0.2)):
    """(verts float32 [(stacks+1) slices, 3], faces int32 [2 stacks slices, 3]): rings of ``slices`` vertices from pole to pole (each pole is
    a ring of coincident vertices, so the 2 ``slices`` faces that touch a pole with two corners have no area), every quad split in two."""
    th = np.pi * np.arange(stacks + 1) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    st, ct = np.sin(th), np.cos(th)
    st[0] = st[-1] = 0.0
    c = np.asarray(centre, np.float64)
    v = np.stack([c[0] + radius * st[:, None] * np.cos(ph)[None], c[1] + radius * ct[:, None] * np.ones_like(ph)[None],
                  c[2] + radius * st[:, None] * np.sin(ph)[None]], -1).reshape(-1, 3).astype(f32)
    faces = []
    for a in range(stacks):
        for b in range(slices):
            p, q, r, s = a * slices + b, a * slices + (b + 1) % slices, (a + 1) * slices + b, (a + 1) * slices + (b + 1) % slices
            faces += [(p, r, q), (q, r, s)]
    return v, np.asarray(faces, np.int32)


def camera(H, W):
    """The off-centre intrinsics of the scenes: fx = fy = 1.1 W, cx = W/2 - 3.25, cy = H/2 + 1.5."""
    return np.array([[1.1 * W, 0, W / 2 - 3.25], [0, 1.1 * W, H / 2 + 1.5], [0, 0, 1]], np.float32)


def scene_a():
    v, f = uv_sphere(12, 16)
    return dict(verts=v, faces=f, H=48, W=64, K=camera(48, 64), c2w=pose34(pose_spherical(25.0, -20.0, 4.0)))


def scene_b(pose=(-40.0, 15.0, 3.5)):
    v, f = uv_sphere(24, 32)
    return dict(verts=v, faces=f, H=29, W=37, K=camera(29, 37), c2w=pose34(pose_spherical(*pose)))


def scene_c():
    """Scene B's sphere under an ANISOTROPIC camera — fx = 1.3 W, fy = 0.8 W, off-centre — with a generic pose (azimuth, elevation, roll and
    a shift off the axis: no rotation entry is 0 or +-1): exchanged focal lengths or principal-point coordinates move every vertex."""
    v, f = uv_sphere(24, 32)
    H, W = 29, 37
    K = np.array([[1.3 * W, 0, W / 2 - 3.25], [0, 0.8 * W, H / 2 + 1.5], [0, 0, 1]], np.float32)
    return dict(verts=v, faces=f, H=H, W=W, K=K, c2w=generic_pose(-40.0, 15.0, 3.5, 20.0, (0.15, -0.1, 0.2)))


def exact_camera(H, W, cx, cy):
    """Identity pose, fx = fy = 16, integer principal point: a vertex (x, y, -1) with dyadic x, y lands at u = cx + 16 x, v = cy - 16 y exactly."""
    return dict(H=H, W=W, K=np.array([[16, 0, cx], [0, 16, cy], [0, 0, 1]], np.float32), c2w=np.eye(4, dtype=np.float32)[:3])


def at_pixels(uv, cx, cy, z=-1.0):
    """World vertices (identity pose, fx = fy = 16) that project exactly onto the pixel coordinates ``uv`` [n,2] at camera depth ``-z``
    (``uv - c`` multiples of 1/16 of small magnitude and ``z`` a power of two keep every step exact)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    depth = -float(z)
    return np.stack([(uv[:, 0] - cx) / 16 * depth, -(uv[:, 1] - cy) / 16 * depth, np.full(len(uv), float(z))], -1).astype(f32)


def quad_scene(n=8, doubled=False):
    """A quad over pixels [2, 2 + n]^2 split along the diagonal through pixel centres (identity pose, exact coordinates); ``doubled``:
    each triangle twice (faces 0, 1 then 2, 3)."""
    cam = exact_camera(n + 5, n + 6, 3.0, 2.0)
    v = at_pixels([(2, 2), (2 + n, 2), (2 + n, 2 + n), (2, 2 + n)], 3.0, 2.0)
    f = [(0, 1, 2), (0, 2, 3)]
    return dict(cam, verts=v, faces=np.asarray(f * (2 if doubled else 1), np.int32))


def behind_scene():
    """Scene A plus one large face BEHIND the camera whose (mirrored) projection covers the image: culled by znear, drawn over every
    background pixel without the cull."""
    s = scene_a()
    c = s["c2w"].astype(np.float64)
    cam = np.array([(-40.0, -40.0, 3.0), (40.0, -40.0, 3.0), (0.0, 60.0, 3.0)])     # camera space, z = +3: behind (the camera looks along -z)
    world = (cam @ c[:, :3].T + c[:, 3]).astype(f32)
    n = len(s["verts"])
    return dict(s, verts=np.concatenate([s["verts"], world]), faces=np.concatenate([s["faces"], np.asarray([(n, n + 1, n + 2)], np.int32)]))
