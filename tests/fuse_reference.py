"""Yardsticks of the depth-map fusion (``mofa_tsdf_*``, ``mesh.tsdf_*``).

* :func:`integrate`, :func:`field` and :func:`depth_frame` restate the kernels and the encoding helper in NumPy, operation for operation:
  the lattice in separately rounded ``np.float32`` steps, everything else in ``np.float64`` on the float32 inputs widened — the GPU state
  must equal it bit for bit, the counters integer for integer.  ``fault`` injects one mistake (``FAULTS``) so that
  tests/test_fuse_reference_cpu.py can show that the comparison catches it.
* :func:`sphere_depth` is the analytic ray-sphere depth (the ray parameter of ``get_rays``) the scenes are built from.
* :func:`catalogue` lists the scenes the CPU and the GPU tests share; :func:`crossings` and :func:`sphere_error` measure a field's surface.
"""
import numpy as np

from rays_reference import pose_spherical

f32, f64 = np.float32, np.float64
FAULTS = ("swap_c", "no_v_flip", "no_transpose", "floor_pixel", "euclidean", "sdf_sign", "no_behind", "no_clamp", "no_carve",
          "unobserved_outside", "no_weights", "fp32_acc", "reverse_views")
UNOBSERVED = ("auto", "outside", "inside")
COUNTS = ("observed", "filled_inside", "filled_outside", "border")
SPHERE_R, SPHERE_C = 1.0, (0.1, -0.05, 0.2)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def axis_coords(n, lo, step):
    """lo + (float)i * step, multiply and add rounded separately in float32 (``mofa_grid_points``)."""
    return (f32(lo) + (np.arange(n).astype(f32) * f32(step)).astype(f32)).astype(f32)


def lattice(res, lo, step):
    """float64 [n,3]: the float32 lattice points widened, in flat index order idx = (i*ny + j)*nz + k."""
    ax = [axis_coords(n, lo[a], step[a]) for a, n in enumerate(res)]
    return np.stack([g.reshape(-1) for g in np.meshgrid(*ax, indexing="ij")], -1).astype(f64)


def new_state(res):
    n = int(np.prod(res))
    return {"acc": np.zeros(n, f64), "wsum": np.zeros(n, f64), "front": np.zeros(n, np.int32), "behind": np.zeros(n, np.int32)}


def cam_table(K, c2w, n_views=1):
    """float32 [n_cams,16]: fx, fy, cx, cy and the 3 x 4 pose per camera; one row when both K and c2w are one camera."""
    K, c = np.asarray(K, f64), np.asarray(c2w, f32)
    Ks, cs = (K[None] if K.ndim == 2 else K), (c[None] if c.ndim == 2 else c)
    n = 1 if len(Ks) == 1 and len(cs) == 1 else n_views
    assert len(Ks) in (1, n) and len(cs) in (1, n)
    rows = []
    for v in range(n):
        k, p = Ks[v % len(Ks)], cs[v % len(cs)]
        rows.append(np.concatenate([np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]], f32), p[:3, :4].astype(f32).reshape(-1)]))
    return np.stack(rows).astype(f32)


def integrate(state, res, lo, step, trunc, depth, cams, weight=None, carve=True, fault=None):
    """One call of ``mofa_tsdf_integrate``: ``depth`` float32 [n,H,W], ``cams`` of :func:`cam_table`, ``weight`` like ``depth`` or None.
    Updates ``state`` in place (and returns it)."""
    assert fault is None or fault in FAULTS
    depth = np.asarray(depth, f32)
    n_views, H, W = depth.shape
    x = lattice(res, lo, step)
    trunc = f64(trunc)
    acc, wsum, front, behind = state["acc"], state["wsum"], state["front"], state["behind"]
    if fault == "fp32_acc":
        acc, wsum = acc.astype(f32), wsum.astype(f32)
    order = range(n_views - 1, -1, -1) if fault == "reverse_views" else range(n_views)
    with np.errstate(all="ignore"):
        for view in order:
            cam = cams[view if len(cams) > 1 else 0].astype(f64)
            fx, fy, cx, cy = cam[:4]
            if fault == "swap_c":
                cx, cy = cy, cx
            c = cam[4:].reshape(3, 4)
            d = [x[:, a] - c[a, 3] for a in range(3)]
            if fault == "no_transpose":
                p = [(d[0] * c[a, 0] + d[1] * c[a, 1]) + d[2] * c[a, 2] for a in range(3)]
            else:
                p = [(d[0] * c[0, a] + d[1] * c[1, a]) + d[2] * c[2, a] for a in range(3)]
            t = -p[2]
            seen = t > 0
            u = cx + fx * (p[0] / t)
            v = (cy + fy * (p[1] / t)) if fault == "no_v_flip" else (cy - fy * (p[1] / t))
            pu, pv = (np.floor(u), np.floor(v)) if fault == "floor_pixel" else (np.floor(u + 0.5), np.floor(v + 0.5))
            seen &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
            iu, iv = np.where(seen, pu, 0).astype(np.int64), np.where(seen, pv, 0).astype(np.int64)
            D = depth[view, iv, iu]
            known = seen & (D > 0)                                     # (NaN, -inf, 0 and negative depths fail)
            background = known & np.isposinf(D)
            surface = known & ~background
            dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) if fault == "euclidean" else t
            sdf = (dist - D.astype(f64)) if fault == "sdf_sign" else (D.astype(f64) - dist)
            is_behind = surface & (sdf < -trunc)
            if fault == "no_behind":
                is_behind = np.zeros_like(is_behind)
            s = sdf / trunc
            if fault != "no_clamp":
                s = np.where(s > 1.0, 1.0, s)
            s = np.where(background, 1.0, s)
            observe = (surface & ~is_behind) | (background & bool(carve and fault != "no_carve"))
            w = np.ones(len(x), f64) if (weight is None or fault == "no_weights") else np.asarray(weight, f32)[view, iv, iu].astype(f64)
            observe &= ~(w == 0)
            behind += is_behind.astype(np.int32)
            front += observe.astype(np.int32)
            if fault == "fp32_acc":
                acc = np.where(observe, (acc + (w.astype(f32) * s.astype(f32)).astype(f32)).astype(f32), acc)
                wsum = np.where(observe, (wsum + w.astype(f32)).astype(f32), wsum)
            else:
                acc[:] = np.where(observe, acc + w * s, acc)
                wsum[:] = np.where(observe, wsum + w, wsum)
    if fault == "fp32_acc":
        state["acc"][:], state["wsum"][:] = acc.astype(f64), wsum.astype(f64)
    return state


def field(state, res, unobserved="auto", close_border=True, fault=None):
    """(field float32 [nx,ny,nz], counts dict) of ``mofa_tsdf_field``."""
    assert unobserved in UNOBSERVED and (fault is None or fault in FAULTS)
    if fault == "unobserved_outside":
        unobserved = "outside"
    acc, wsum, behind = state["acc"], state["wsum"], state["behind"]
    observed = wsum > 0
    inside = {"auto": behind > 0, "outside": np.zeros(len(acc), bool), "inside": np.ones(len(acc), bool)}[unobserved]
    with np.errstate(all="ignore"):
        out = np.where(observed, (-(acc / wsum)).astype(f32), np.where(inside, f32(1), f32(-1))).astype(f32).reshape(res)
    counts = {"observed": int(observed.sum()), "filled_inside": int((~observed & inside).sum()),
              "filled_outside": int((~observed & ~inside).sum()), "border": 0}
    if close_border:
        edge = np.zeros(res, bool)
        for a in range(3):
            sl = [slice(None)] * 3
            for end in (0, -1):
                sl[a] = end
                edge[tuple(sl)] = True
        out[edge] = f32(-1)
        counts["border"] = int(edge.sum())
    return out, counts


def depth_frame(depth, mask, background="empty"):
    """The encoding ``mofa_tsdf_integrate`` reads: ``depth`` where ``mask``, +inf (``"empty"``) or NaN (``"unknown"``) elsewhere."""
    fill = {"empty": f32(np.inf), "unknown": f32(np.nan)}[background]
    return np.where(np.asarray(mask, bool), np.asarray(depth, f32), fill).astype(f32)


def fuse(case, fault=None, batches=None):
    """The state of a catalogue entry after all its frames, integrated in ``batches`` (a list of view counts; None: one call)."""
    n = len(case["depth"])
    state = new_state(case["res"])
    first = 0
    for b in (batches or [n]):
        sl = slice(first, first + b)
        cams = case["cams"] if len(case["cams"]) == 1 else case["cams"][sl]
        integrate(state, case["res"], case["lo"], case["step"], case["trunc"], case["depth"][sl], cams,
                  None if case["weight"] is None else case["weight"][sl], case["carve"], fault)
        first += b
    assert first == n
    return state


# ---- analytic depth --------------------------------------------------------------------------------------------------------------------
def rays64(H, W, cam):
    """(o [3], d [H,W,3]) in float64 from one row of :func:`cam_table`: the rays of ``get_rays``, d = R [(i - cx) / fx, -(j - cy) / fy, -1]."""
    cam = np.asarray(cam, f64)
    fx, fy, cx, cy = cam[:4]
    c = cam[4:].reshape(3, 4)
    i, j = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64), indexing="xy")
    d = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1) @ c[:, :3].T
    return c[:, 3], d


def sphere_depth(H, W, cam, centre=SPHERE_C, radius=SPHERE_R, far_side=False):
    """float32 [H,W]: the ray parameter of the first (``far_side``: the last) intersection with the sphere, +inf on misses."""
    o, d = rays64(H, W, cam)
    oc = o - np.asarray(centre, f64)
    a, b, c = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - radius * radius
    disc = b * b - a * c
    with np.errstate(all="ignore"):
        t = (-b + (1 if far_side else -1) * np.sqrt(disc)) / a
    return np.where((disc >= 0) & (t > 0), t, np.inf).astype(f32)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def grid_of(res, lo, hi):
    """(res, lo, step) as ``mesh.grid_spec`` computes them (float32)."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    return tuple(res), lo, ((hi - lo) / (np.asarray(res, f32) - f32(1))).astype(f32)


SPHERE_H, SPHERE_W = 40, 56


def sphere_camera(H=SPHERE_H, W=SPHERE_W):
    """Anisotropic, non-square and off-centre: fx = 0.975 W, fy = 0.96 W, cx = W/2 - 3.25, cy = H/2 + 1.5."""
    return np.array([[0.975 * W, 0, W / 2 - 3.25], [0, 0.96 * W, H / 2 + 1.5], [0, 0, 1]], f32)


def sphere_poses():
    """Eight look-at poses at distance 4 from the sphere's centre: six around it at azimuth -180 + 60 k degrees, elevation -25 (even k) or
    +20 (odd k), and two at elevation +-89."""
    views = [(-180.0 + 60.0 * k, -25.0 if k % 2 == 0 else 20.0) for k in range(6)] + [(0.0, 89.0), (0.0, -89.0)]
    return np.stack([pose_spherical(az, el, 4.0, shift=SPHERE_C) for az, el in views]).astype(f32)


def _case(name, grid, trunc, depth, cams, weight=None, carve=True):
    res, lo, step = grid
    return dict(name=name, res=res, lo=lo, step=step, trunc=float(trunc), depth=np.ascontiguousarray(depth, f32), cams=cams,
                weight=None if weight is None else np.ascontiguousarray(weight, f32), carve=carve)


def sphere_scene(H=SPHERE_H, W=SPHERE_W, carve=True, name="sphere"):
    """The quality scene: R = 1 at (0.1, -0.05, 0.2), 33^3 over centre +- 1.3, trunc = 3 steps, the eight poses, analytic depth."""
    c = np.asarray(SPHERE_C, f64)
    grid = grid_of((33, 33, 33), c - 1.3, c + 1.3)
    cams = cam_table(sphere_camera(H, W), sphere_poses(), 8)
    depth = np.stack([sphere_depth(H, W, cam) for cam in cams])
    return _case(name, grid, 3.0 * float(grid[2][0]), depth, cams, carve=carve)


EXACT = dict(H=20, W=24, cx=12.0, cy=10.0, res=(9, 9, 9), lo=(-0.5, -0.5, -3.0), step=(0.125, 0.125, 0.25), trunc=0.5,
             depths=(2.0, 2.25), weights=(1.0, 2.0))


def exact_scene():
    """Identity pose at the origin, fx = fy = 16, integer principal point; the lattice has dyadic coordinates with t = -z in [1, 3] and every
    voxel projects into the frame; two constant-depth frames (2 and 2.25) with constant weights 1 and 2, trunc = 1/2: every s is dyadic,
    s_f = min((D_f - t) / 0.5, 1), and t > D_f + 0.5 lies behind."""
    e = EXACT
    K = np.array([[16, 0, e["cx"]], [0, 16, e["cy"]], [0, 0, 1]], f32)
    cams = cam_table(K, np.eye(4, dtype=f32)[:3], 2)
    depth = np.stack([np.full((e["H"], e["W"]), d, f32) for d in e["depths"]])
    weight = np.stack([np.full((e["H"], e["W"]), w, f32) for w in e["weights"]])
    grid = (e["res"], np.asarray(e["lo"], f32), np.asarray(e["step"], f32))
    return _case("exact", grid, e["trunc"], depth, cams, weight)


def exact_expected():
    """(acc, wsum, front, behind) of :func:`exact_scene` in closed form, per lattice point in flat order."""
    e = EXACT
    z = e["lo"][2] + np.arange(e["res"][2]) * e["step"][2]
    t = np.broadcast_to(-z, e["res"]).reshape(-1)
    acc, wsum = np.zeros(len(t)), np.zeros(len(t))
    front, behind = np.zeros(len(t), np.int32), np.zeros(len(t), np.int32)
    for D, w in zip(e["depths"], e["weights"]):
        back = D - t < -e["trunc"]
        s = np.minimum((D - t) / e["trunc"], 1.0)
        acc += np.where(back, 0.0, w * s)
        wsum += np.where(back, 0.0, w)
        front += ~back
        behind += back
    return acc, wsum, front, behind


def view_order_scene():
    """The exact camera with three constant frames (2, 2.5, 2.375) weighted (2^60, 2^60, 1): on the plane t = 2.25 the first two
    observations are -1/2 and +1/2 and cancel exactly, so in order acc = 1/4 there, while any order that meets the small term first loses it
    in a sum of magnitude 2^59: the sequential fp64 sum in view order is visible in the FIELD, not only in the last bits of the state."""
    e = EXACT
    K = np.array([[16, 0, e["cx"]], [0, 16, e["cy"]], [0, 0, 1]], f32)
    depth = np.stack([np.full((e["H"], e["W"]), d, f32) for d in (2.0, 2.5, 2.375)])
    weight = np.stack([np.full((e["H"], e["W"]), w, f32) for w in (2.0 ** 60, 2.0 ** 60, 1.0)])
    grid = (e["res"], np.asarray(e["lo"], f32), np.asarray(e["step"], f32))
    return _case("view_order", grid, e["trunc"], depth, cam_table(K, np.eye(4, dtype=f32)[:3], 3), weight)


def catalogue():
    """The scenes the CPU and the GPU tests share (each a dict: name, res, lo, step, trunc, depth [n,H,W], cams, weight, carve)."""
    out = [sphere_scene(), exact_scene()]
    c = np.asarray(SPHERE_C, f64)
    H, W = 23, 31
    K = np.array([[30.0, 0, W / 2 - 1.25], [0, 27.5, H / 2 + 0.75], [0, 0, 1]], f32)
    poses = np.stack([pose_spherical(az, el, 3.5, roll, shift=SPHERE_C) for az, el, roll in ((35.0, -20.0, 12.0), (-100.0, 30.0, -17.0),
                                                                                              (160.0, 5.0, 40.0))]).astype(f32)
    cams = cam_table(K, poses, 3)
    depth = np.stack([sphere_depth(H, W, cam, radius=0.8) for cam in cams])
    # a non-cubic lattice with three different steps
    out.append(_case("non_cubic", grid_of((9, 17, 33), c - (0.9, 1.1, 1.3), c + (1.0, 1.2, 1.1)), 0.2, depth, cams))
    # the camera sits inside the volume: voxels behind it (t <= 0) and voxels that project out of the small frame; one K, one pose
    inside_cam = cam_table(np.array([[9.0, 0, 6.5], [0, 11.0, 4.25], [0, 0, 1]], f32), pose_spherical(25.0, -15.0, 0.3, 10.0, shift=SPHERE_C), 2)
    inner = np.stack([sphere_depth(9, 13, inside_cam[0], radius=r, far_side=True) for r in (0.9, 0.7)])
    out.append(_case("camera_inside", grid_of((17, 15, 13), c - 1.2, c + 1.2), 0.25, inner, inside_cam))
    # every depth class in one frame: NaN, -inf, 0, negative, +inf next to real depths
    classes = depth[:2].copy()
    classes[0, 2:6, 3:9], classes[0, 8:11, 12:20], classes[0, 14:18, 5:15] = np.nan, -np.inf, 0.0
    classes[1, 3:9, 10:22], classes[1, 12:20, 8:16] = -1.5, np.inf
    out.append(_case("depth_classes", grid_of((15, 15, 15), c - 1.1, c + 1.1), 0.3, classes, cams[:2]))
    # a weight map with zeros (and weights that are no powers of two)
    rng = np.random.default_rng(7)
    weight = rng.choice(np.array([0.0, 0.3, 1.0, 2.25], f32), size=depth.shape).astype(f32)
    out.append(_case("weights", grid_of((15, 14, 13), c - 1.1, c + 1.1), 0.3, depth, cams, weight))
    # truncation extremes: below one step, and larger than the volume
    out.append(_case("trunc_small", grid_of((15, 15, 15), c - 1.1, c + 1.1), 0.4 * 2.2 / 14, depth, cams))
    out.append(_case("trunc_large", grid_of((15, 15, 15), c - 1.1, c + 1.1), 10.0, depth, cams))
    # carving off: the background says nothing
    out.append(_case("no_carving", grid_of((15, 15, 15), c - 1.1, c + 1.1), 0.3, depth, cams, carve=False))
    out.append(view_order_scene())
    return out


# ---- measuring a field's surface -------------------------------------------------------------------------------------------------------
def crossings(fld, res, lo, step):
    """float64 [n,3]: the zero crossings of the field on the lattice's axis edges, by linear interpolation between the two ends."""
    fld = np.asarray(fld, f64)
    ax = [axis_coords(n, lo[a], step[a]).astype(f64) for a, n in enumerate(res)]
    pts = []
    for a in range(3):
        lo_sl, hi_sl = [slice(None)] * 3, [slice(None)] * 3
        lo_sl[a], hi_sl[a] = slice(0, -1), slice(1, None)
        fa, fb = fld[tuple(lo_sl)], fld[tuple(hi_sl)]
        idx = np.argwhere((fa >= 0) != (fb >= 0))
        t = fa[tuple(idx.T)] / (fa[tuple(idx.T)] - fb[tuple(idx.T)])
        p = np.stack([ax[b][idx[:, b]] for b in range(3)], -1)
        p[:, a] += t * (ax[a][idx[:, a] + 1] - ax[a][idx[:, a]])
        pts.append(p)
    return np.concatenate(pts)


def sphere_error(points, step, centre=SPHERE_C, radius=SPHERE_R):
    """| |p - c| - R | in grid steps (the largest of the three), float64 [n]."""
    r = np.linalg.norm(np.asarray(points, f64) - np.asarray(centre, f64), axis=1)
    return np.abs(r - radius) / float(np.max(np.asarray(step, f64)))
