"""Yardsticks of the multi-view colour baking (``mofa_bake_*``, ``mesh.bake_*`` / ``fill_colors``).

* :func:`integrate`, :func:`resolve` and :func:`fill_step` restate the three kernels in NumPy, operation for operation, in ``np.float64`` on
  the float32 inputs widened — the GPU state and colours must equal them bit for bit, the counters integer for integer.  ``fault`` injects
  one mistake (``FAULTS``) so that tests/test_bake_reference_cpu.py can show that the comparison catches it.
* :func:`new_state`, :func:`bake`, :func:`resolve` and :func:`fill_colors` stand for the four ``mesh`` calls.
* :func:`catalogue` lists the scenes the CPU and the GPU tests share; cameras and meshes come from tests/raster_reference.py, depth frames
  (and the rasterised images) from its NumPy ``rasterize``.
"""
import numpy as np

import raster_reference as rast
from fuse_reference import cam_table, depth_frame, same_bits  # noqa: F401  (re-exported for the tests)
from rays_reference import pose_spherical

f32, f64 = np.float32, np.float64
FAULTS = ("swap_uv", "no_v_flip", "nearest", "round_footprint", "one_corner_depth", "abs_depth", "background_visible", "cos_unnormalised",
          "power_off_by_one", "best_tie_late", "csum_unweighted", "fill_in_place", "fill_by_degree")
COUNTS = ("colored", "occluded", "grazing", "unseen")
STATE_KEYS = ("csum", "wsum", "wbest", "cbest", "seen", "occluded", "grazing")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def new_state(V, C=3):
    return {"csum": np.zeros((V, C), f64), "wsum": np.zeros(V, f64), "wbest": np.zeros(V, f64), "cbest": np.zeros((V, C), f32),
            "seen": np.zeros(V, np.int32), "occluded": np.zeros(V, np.int32), "grazing": np.zeros(V, np.int32)}


def integrate(state, verts, images, depth, cams, normals=None, *, depth_tol, cos_min=0.0, power=2, fault=None):
    """One call of ``mofa_bake_integrate``: ``verts`` float32 [V,3], ``images`` float32 [n,H,W,C], ``depth`` float32 [n,H,W], ``cams`` of
    ``cam_table``, ``normals`` float32 [V,3] or None.  Updates ``state`` in place (and returns it)."""
    assert fault is None or fault in FAULTS
    x = np.asarray(verts, f32).astype(f64)
    images, depth = np.asarray(images, f32), np.asarray(depth, f32)
    n_views, H, W, C = images.shape
    assert depth.shape == (n_views, H, W) and state["csum"].shape == (len(x), C)
    n = None if normals is None else np.asarray(normals, f32).astype(f64)
    depth_tol, cos_min = f64(depth_tol), f64(cos_min)
    csum, wsum, wbest, cbest = state["csum"], state["wsum"], state["wbest"], state["cbest"]
    with np.errstate(all="ignore"):
        for view in range(n_views):
            cam = cams[view if len(cams) > 1 else 0].astype(f64)
            fx, fy, cx, cy = cam[:4]
            c = cam[4:].reshape(3, 4)
            d = [x[:, a] - c[a, 3] for a in range(3)]
            p = [(d[0] * c[0, a] + d[1] * c[1, a]) + d[2] * c[2, a] for a in range(3)]
            t = -p[2]
            live = t > 0
            u = cx + fx * (p[0] / t)
            v = (cy + fy * (p[1] / t)) if fault == "no_v_flip" else (cy - fy * (p[1] / t))
            if fault == "swap_uv":
                u, v = v, u
            u0, v0 = (np.floor(u + 0.5), np.floor(v + 0.5)) if fault == "round_footprint" else (np.floor(u), np.floor(v))
            live &= (u0 >= 0) & (u0 + 1 <= W - 1) & (v0 >= 0) & (v0 + 1 <= H - 1)         # (a non-finite value fails)
            iu, iv = np.where(live, u0, 0).astype(np.int64), np.where(live, v0, 0).astype(np.int64)
            at = ((iv, iu), (iv, iu + 1), (iv + 1, iu), (iv + 1, iu + 1))                  # the footprint's corners 00, 10, 01, 11
            D = [depth[view, j, i] for j, i in at]
            tested = D[:1] if fault == "one_corner_depth" else D
            known = np.logical_and.reduce([k > 0 for k in tested])                          # (NaN, -inf, 0 and negative depths fail)
            background = np.logical_or.reduce([np.isposinf(k) for k in tested])
            if fault == "background_visible":
                background = np.zeros_like(background)
            live &= known & ~background
            diff = [t - k.astype(f64) for k in tested]
            if fault == "abs_depth":
                diff = [np.abs(k) for k in diff]
            occ = live & np.logical_or.reduce([k > depth_tol for k in diff])
            state["occluded"] += occ.astype(np.int32)
            live &= ~occ
            w = np.ones(len(x), f64)
            if n is not None:
                e = [-d[a] for a in range(3)]
                dot = (n[:, 0] * e[0] + n[:, 1] * e[1]) + n[:, 2] * e[2]
                cosv = dot if fault == "cos_unnormalised" else dot / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                graze = live & ~(cosv > cos_min)
                state["grazing"] += graze.astype(np.int32)
                live &= ~graze
                for _ in range(power + (1 if fault == "power_off_by_one" else 0)):
                    w = w * cosv
            fu, fv = u - u0, v - v0
            if fault == "nearest":
                fu, fv = np.floor(fu + 0.5), np.floor(fv + 0.5)
            tex = [images[view, j, i] for j, i in at]                                       # float32 [V,C] each
            live &= np.logical_and.reduce([np.isfinite(k).all(-1) for k in tex])
            c00, c10, c01, c11 = (k.astype(f64) for k in tex)
            a = c00 + fu[:, None] * (c10 - c00)
            b = c01 + fu[:, None] * (c11 - c01)
            col = a + fv[:, None] * (b - a)
            term = col if fault == "csum_unweighted" else w[:, None] * col
            csum[:] = np.where(live[:, None], csum + term, csum)
            wsum[:] = np.where(live, wsum + w, wsum)
            state["seen"] += live.astype(np.int32)
            best = live & ((w >= wbest) if fault == "best_tie_late" else (w > wbest))
            wbest[:] = np.where(best, w, wbest)
            cbest[:] = np.where(best[:, None], col.astype(f32), cbest)
    return state


def resolve(state, blend="mean", fill=0.0):
    """dict of ``mofa_bake_resolve`` / ``mesh.bake_colors``: ``colors`` float32 [V,C], ``valid`` bool [V], ``counts``, ``seen``."""
    assert blend in ("mean", "best")
    ok = (state["wsum"] > 0) if blend == "mean" else (state["seen"] > 0)
    with np.errstate(all="ignore"):
        col = (state["csum"] / state["wsum"][:, None]).astype(f32) if blend == "mean" else state["cbest"]
    colors = np.where(ok[:, None], col, f32(fill)).astype(f32)
    occ, graze = state["occluded"] > 0, state["grazing"] > 0
    counts = {"colored": int(ok.sum()), "occluded": int((~ok & occ).sum()), "grazing": int((~ok & ~occ & graze).sum()),
              "unseen": int((~ok & ~occ & ~graze).sum())}
    return {"colors": colors, "valid": ok, "counts": counts, "seen": state["seen"]}


def adjacency(faces, V):
    """Per vertex the ascending list of its distinct neighbours without itself (``mesh.vertex_adjacency``'s order)."""
    sets = [set() for _ in range(V)]
    for tri in np.asarray(faces, np.int64).reshape(-1, 3):
        for p, q in ((0, 1), (1, 2), (2, 0)):
            if tri[p] != tri[q]:
                sets[tri[p]].add(int(tri[q]))
                sets[tri[q]].add(int(tri[p]))
    return [sorted(s) for s in sets]


def fill_step(colors, valid, nbrs, fault=None):
    """One step of ``mofa_bake_fill``: (colors float32 [V,C], valid bool [V]) from the INPUT arrays."""
    src_c, src_v = colors, valid
    out_c, out_v = colors.copy(), valid.copy()
    if fault == "fill_in_place":
        src_c, src_v = out_c, out_v
    for i, js in enumerate(nbrs):
        if valid[i]:
            continue
        good = [j for j in js if src_v[j]]
        if not good:
            continue
        s = np.zeros(colors.shape[1], f64)
        for j in good:
            s = s + src_c[j].astype(f64)
        out_c[i] = (s / f64(len(js) if fault == "fill_by_degree" else len(good))).astype(f32)
        out_v[i] = True
    return out_c, out_v


def fill_colors(colors, valid, faces, iterations, fault=None):
    """(colors, valid, remaining) of ``mesh.fill_colors``."""
    colors, valid = np.asarray(colors, f32).copy(), np.asarray(valid, bool).copy()
    nbrs = adjacency(faces, len(colors))
    for _ in range(iterations):
        colors, valid = fill_step(colors, valid, nbrs, fault)
    return colors, valid, int((~valid).sum())


def bake(case, fault=None, batches=None):
    """The state of a catalogue entry after all its frames, integrated in ``batches`` (a list of view counts; None: one call)."""
    n = len(case["depth"])
    state = new_state(len(case["verts"]), case["images"].shape[-1])
    first = 0
    for b in (batches or [n]):
        if b == 0:
            continue
        sl = slice(first, first + b)
        cams = case["cams"] if len(case["cams"]) == 1 else case["cams"][sl]
        integrate(state, case["verts"], case["images"][sl], case["depth"][sl], cams, case["normals"], depth_tol=case["depth_tol"],
                  cos_min=case["cos_min"], power=case["power"], fault=fault)
        first += b
    assert first == n
    return state


# ---- scene pieces ----------------------------------------------------------------------------------------------------------------------
def _case(name, verts, images, depth, cams, normals=None, depth_tol=0.25, cos_min=0.0, power=2, faces=None, **extra):
    images, depth = np.ascontiguousarray(images, f32), np.ascontiguousarray(depth, f32)
    assert images.ndim == 4 and depth.shape == images.shape[:3]
    return dict(name=name, verts=np.ascontiguousarray(verts, f32).reshape(-1, 3), images=images, depth=depth, cams=np.ascontiguousarray(cams, f32),
                normals=None if normals is None else np.ascontiguousarray(normals, f32).reshape(-1, 3), depth_tol=float(depth_tol),
                cos_min=float(cos_min), power=int(power), faces=None if faces is None else np.ascontiguousarray(faces, np.int32), **extra)


def pow2_image(H, W, C=3, shift=0):
    """float32 [H,W,C] of powers of two: 2^((3 i + 5 j + 2 ch + shift) mod 7): sums and halves of a few of them are exact."""
    j, i, ch = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return (2.0 ** ((3 * i + 5 * j + 2 * ch + shift) % 7)).astype(f32)


def grid_quad(u_lo, v_lo, u_hi, v_hi, nu, nv, cx, cy, z=-1.0):
    """(verts [(nv+1)(nu+1),3], faces, uv): a fronto-parallel quad under the exact camera whose (nu+1) x (nv+1) vertices project exactly
    onto the pixel coordinates u_lo .. u_hi, v_lo .. v_hi (row-major in v), every cell split in two."""
    us, vs = np.linspace(u_lo, u_hi, nu + 1), np.linspace(v_lo, v_hi, nv + 1)
    uv = np.stack(np.meshgrid(us, vs, indexing="xy"), -1).reshape(-1, 2)
    faces = []
    for b in range(nv):
        for a in range(nu):
            p, q, r, s = b * (nu + 1) + a, b * (nu + 1) + a + 1, (b + 1) * (nu + 1) + a, (b + 1) * (nu + 1) + a + 1
            faces += [(p, r, q), (q, r, s)]
    return rast.at_pixels(uv, cx, cy, z), np.asarray(faces, np.int32), uv


def raster_frame(verts, faces, cam, attrs=None):
    """(depth frame float32 [H,W] in depth_frame's encoding, attr float32 [H,W,C] or None) of the NumPy rasteriser."""
    r = rast.rasterize(verts, faces, cam["H"], cam["W"], cam["K"], cam["c2w"], attrs=attrs)
    return depth_frame(r["depth"], r["face"] >= 0), (None if attrs is None else r["attr"])


EXACT = dict(H=12, W=14, cx=7.0, cy=6.0)


def exact_camera():
    return rast.exact_camera(EXACT["H"], EXACT["W"], EXACT["cx"], EXACT["cy"])


def exact_cams(n=1):
    cam = exact_camera()
    return cam_table(cam["K"], cam["c2w"], n)


def exact_uv():
    """The exact scene's vertices in pixel coordinates: on pixels, on half pixels in u, in v and in both, all with the footprint inside."""
    return np.array([(3, 2), (0, 0), (12, 10), (7, 6), (3.5, 2), (11.5, 9), (3, 2.5), (0, 9.5), (3.5, 2.5), (11.5, 9.5), (0.5, 0.5)], f64)


def exact_scene():
    """The plane z = -1 seen by the identity camera with fx = fy = 16 (depth 1 at every pixel), a powers-of-two image and vertices that
    project exactly onto pixels and half pixels: the colour is the texel, or the exact mean of two or of four texels; no normals: w = 1."""
    e = EXACT
    verts = rast.at_pixels(exact_uv(), e["cx"], e["cy"])
    return _case("exact", verts, pow2_image(e["H"], e["W"])[None], np.ones((1, e["H"], e["W"]), f32), exact_cams(), uv=exact_uv())


def exact_expected():
    """float64 [V,3]: the exact scene's colours in closed form."""
    img = pow2_image(EXACT["H"], EXACT["W"]).astype(f64)
    out = []
    for u, v in exact_uv():
        i, j = int(np.floor(u)), int(np.floor(v))
        cols = [img[j, i]]
        if u != i:
            cols.append(img[j, i + 1])
        if v != j:
            cols += [img[j + 1, k] for k in ((i, i + 1) if u != i else (i,))]
        out.append(sum(cols) / len(cols))
    return np.asarray(out)


OCCLUSION = dict(H=17, W=18, cx=8.0, cy=8.0, back=(2, 14), front=(6, 10))


def occlusion_scene():
    """A 4 x 4-pixel quad at depth 1 in front of a 12 x 12-pixel quad at depth 2 whose 13 x 13 vertices sit on the pixels 2 .. 14: the
    back vertices whose footprint {u, u + 1} x {v, v + 1} touches a pixel of the front quad (6 .. 10) are occluded, those on the back
    quad's last row and column (14) reach over the silhouette.  The image is the mesh's own rasterised colours."""
    o = OCCLUSION
    cam = rast.exact_camera(o["H"], o["W"], o["cx"], o["cy"])
    vb, fb, uvb = grid_quad(o["back"][0], o["back"][0], o["back"][1], o["back"][1], 12, 12, o["cx"], o["cy"], z=-2.0)
    vf, ff, uvf = grid_quad(o["front"][0], o["front"][0], o["front"][1], o["front"][1], 1, 1, o["cx"], o["cy"], z=-1.0)
    verts, faces = np.concatenate([vb, vf]), np.concatenate([fb, ff + len(vb)])
    attrs = np.concatenate([np.stack([uvb[:, 0] / 16, uvb[:, 1] / 16, np.full(len(uvb), 0.25)], -1),
                            np.stack([np.full(len(uvf), 1.0), uvf[:, 0] / 16, uvf[:, 1] / 16], -1)]).astype(f32)
    depth, image = raster_frame(verts, faces, cam, attrs)
    return _case("occlusion", verts, image[None], depth[None], cam_table(cam["K"], cam["c2w"]), depth_tol=0.5, faces=faces,
                 uv=np.concatenate([uvb, uvf]), n_back=len(vb))


def depth_classes_scene():
    """The exact plane with one pixel each of background (+inf), NaN, a negative depth, zero and -inf: a vertex is skipped when the pixel is
    ANY of the four corners of its footprint.  Vertices on every pixel 0 .. W-2, 0 .. H-2."""
    e = EXACT
    depth = np.ones((1, e["H"], e["W"]), f32)
    bad = {(2, 2): np.inf, (5, 3): np.nan, (9, 4): -1.5, (3, 8): 0.0, (10, 9): -np.inf}                   # (i, j): value
    for (i, j), value in bad.items():
        depth[0, j, i] = value
    uv = np.stack(np.meshgrid(np.arange(e["W"] - 1), np.arange(e["H"] - 1), indexing="xy"), -1).reshape(-1, 2).astype(f64)
    return _case("depth_classes", rast.at_pixels(uv, e["cx"], e["cy"]), pow2_image(e["H"], e["W"])[None], depth, exact_cams(), uv=uv, bad=bad)


ANGLE = dict(H=24, W=40, cx=20.0, cy=12.0, cos_min=0.5, angles=(40.0, 72.0))


def tilted_grid(centre, angle_deg, half, n):
    """(verts float32 [(n+1)^2,3], faces, unit normal float32 [3]): a square of half-width ``half`` around ``centre``, turned by
    ``angle_deg`` about the vertical axis through its centre; the normal is the side that faces a camera at the origin for |angle| < 90."""
    a = np.deg2rad(angle_deg)
    s = np.linspace(-half, half, n + 1)
    g = np.stack(np.meshgrid(s, s, indexing="xy"), -1).reshape(-1, 2)
    verts = np.asarray(centre, f64) + np.stack([g[:, 0] * np.cos(a), g[:, 1], g[:, 0] * np.sin(a)], -1)
    faces = []
    for b in range(n):
        for q in range(n):
            p0, p1, p2, p3 = b * (n + 1) + q, b * (n + 1) + q + 1, (b + 1) * (n + 1) + q, (b + 1) * (n + 1) + q + 1
            faces += [(p0, p2, p1), (p1, p2, p3)]
    return verts.astype(f32), np.asarray(faces, np.int32), np.array([-np.sin(a), 0.0, np.cos(a)], f32)


def _turn(centre, desired_deg, side):
    """The angle of :func:`tilted_grid` at which the quad's normal makes ``desired_deg`` with the direction from ``centre`` to a camera at
    the origin (``side`` = -1 / +1: turned toward -x / +x of it)."""
    phi = np.rad2deg(np.arctan2(-centre[0], -centre[2]))
    return -(phi + side * desired_deg)


def angle_scene(power):
    """Two small quads before the identity camera (fx = fy = 48), turned about the vertical until their normals make 40 and 72 degrees with
    the direction to the camera at their centres (+- 9 degrees over a quad): with cos_min = 0.5 the first passes the angle test and weighs
    cos^power, the second (cos 0.15 .. 0.45) is rejected as grazing.  Normals are the quads' own."""
    g = ANGLE
    cam = dict(H=g["H"], W=g["W"], K=np.array([[48, 0, g["cx"]], [0, 48, g["cy"]], [0, 0, 1]], f32), c2w=np.eye(4, dtype=f32)[:3])
    ca, cb = (-0.45, 0.02, -2.0), (0.45, -0.02, -2.2)
    va, fa, na = tilted_grid(ca, _turn(ca, g["angles"][0], -1), 0.3, 8)
    vb, fb, nb = tilted_grid(cb, _turn(cb, g["angles"][1], +1), 0.3, 8)
    verts, faces = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])
    normals = np.concatenate([np.tile(na, (len(va), 1)), np.tile(nb, (len(vb), 1))])
    attrs = (verts * f32(0.3) + f32(0.5)).astype(f32)
    depth, image = raster_frame(verts, faces, cam, attrs)
    return _case(f"angle_power{power}", verts, image[None], depth[None], cam_table(cam["K"], cam["c2w"]), normals, depth_tol=0.5,
                 cos_min=g["cos_min"], power=power, faces=faces, n_first=len(va))


def best_tie_scene():
    """Two views of the exact scene with different images and no normals: both weigh 1, and `best` keeps the FIRST."""
    e = EXACT
    images = np.stack([pow2_image(e["H"], e["W"]), pow2_image(e["H"], e["W"], shift=3)])
    return _case("best_tie", rast.at_pixels(exact_uv(), e["cx"], e["cy"]), images, np.ones((2, e["H"], e["W"]), f32), exact_cams(), uv=exact_uv())


def view_order_scene():
    """Three views of the exact scene with constant images 2^60, -2^60 and 1 (every weight 1): in order csum = (2^60 - 2^60) + 1 = 1 and
    the mean is 1/3; any order that meets the 1 before the cancellation loses it in a sum of magnitude 2^60."""
    e = EXACT
    images = np.stack([np.full((e["H"], e["W"], 3), k, f32) for k in (2.0 ** 60, -(2.0 ** 60), 1.0)])
    return _case("view_order", rast.at_pixels(exact_uv(), e["cx"], e["cy"]), images, np.ones((3, e["H"], e["W"]), f32), exact_cams(), uv=exact_uv())


def _ball(stacks=6, slices=8):
    v, f = rast.uv_sphere(stacks, slices, radius=0.8)
    n = (v.astype(f64) - np.asarray((0.1, -0.05, 0.2)))
    return v, f, (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)).astype(f32)


GENERIC_POSES = ((35.0, -20.0, 3.5, 12.0), (-100.0, 30.0, 3.5, -17.0), (160.0, 5.0, 3.5, 40.0))


def generic_scene(name, C=3, H=23, W=31, n_views=3, one_camera=False, seed=11, V=None, **params):
    """A small UV sphere (or ``V`` random points around it, with random unit normals) under ``n_views`` generic cameras — anisotropic,
    off-centre, rolled — with the sphere's rasterised depth and RANDOM images of ``C`` channels (nothing is exact here: the scene is for
    the bit-for-bit comparison).  ``one_camera``: every view from the first pose (n_cams = 1)."""
    rng = np.random.default_rng(seed)
    verts, faces, normals = _ball()
    K = np.array([[1.3 * W, 0, W / 2 - 1.25], [0, 1.1 * W, H / 2 + 0.75], [0, 0, 1]], f32)
    poses = [pose_spherical(az, el, r, roll, shift=(0.1, -0.05, 0.2)) for az, el, r, roll in GENERIC_POSES[:n_views]]
    if one_camera:
        poses = poses[:1]
    depth = [raster_frame(verts, faces, dict(H=H, W=W, K=K, c2w=p))[0] for p in poses]
    depth = np.stack(depth * (n_views if one_camera else 1))
    images = rng.uniform(-1.0, 2.0, (n_views, H, W, C)).astype(f32)
    bake_verts, bake_normals = verts, normals
    if V is not None:
        dirs = rng.normal(size=(V, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        bake_verts = (np.asarray((0.1, -0.05, 0.2)) + dirs * rng.uniform(0.7, 0.8, (V, 1))).astype(f32)
        turn = dirs + 0.4 * rng.normal(size=(V, 3))
        bake_normals = (turn / np.linalg.norm(turn, axis=1, keepdims=True)).astype(f32)
    return _case(name, bake_verts, images, depth, cam_table(K, np.stack(poses), n_views), bake_normals, faces=faces if V is None else None,
                 **dict(dict(depth_tol=0.2, cos_min=0.6, power=2), **params))


def bounds_scene():
    """The exact plane with vertices that must not be read: behind the camera, at u = W - 1 exactly, at v = H - 1 exactly, just below u = 0
    and v = 0, far outside, NaN and infinite coordinates — and vertices whose footprint holds a NaN or an infinite TEXEL (skipped: the state
    stays finite).  The first vertices are ordinary, so something is seen."""
    e = EXACT
    H, W = e["H"], e["W"]
    ok = [(3, 2), (6.25, 7.5), (W - 2, H - 2), (W - 1.0009765625, H - 1.0009765625)]
    off = [(W - 1, 4), (4, H - 1), (-0.0009765625, 4), (4, -0.0009765625), (-1, -1), (W, H), (1e6, 3), (3, -1e6)]
    verts = rast.at_pixels(ok + off, e["cx"], e["cy"])
    behind = rast.at_pixels([(3, 2), (7, 6)], e["cx"], e["cy"]) * f32(-1)                                 # z = +1: behind the camera
    wild = np.array([(np.nan, 0, -1), (0, np.inf, -1), (0, 0, np.nan), (-np.inf, 0, -1), (0, 0, -np.inf), (0, 0, 0)], f32)
    image = pow2_image(H, W)
    image[8, 3, 1], image[5, 10, 2] = np.nan, np.inf
    texel = rast.at_pixels([(3, 8), (2.5, 7.5), (10, 5), (9.25, 4.75), (10, 4)], e["cx"], e["cy"])        # each footprint holds one of the two
    return _case("image_bounds", np.concatenate([verts, behind, wild, texel]), image[None], np.ones((1, H, W), f32), exact_cams(),
                 n_ok=len(ok), n_texel=len(texel))


def smallest_frame_scene():
    """A 2 x 2 frame: the only footprint is the whole frame, u and v in [0, 1)."""
    cam = rast.exact_camera(2, 2, 1.0, 1.0)
    uv = [(0, 0), (0.5, 0.5), (0.999, 0.25), (1, 0), (0, 1), (1, 1), (-0.001, 0.5)]
    image = np.array([[[1, 2, 4], [8, 16, 32]], [[64, 128, 256], [512, 1024, 2048]]], f32)
    return _case("frame_2x2", rast.at_pixels(uv, 1.0, 1.0), image[None], np.ones((1, 2, 2), f32), cam_table(cam["K"], cam["c2w"]), n_inside=3)


SPHERE = dict(H=40, W=56, stacks=12, slices=16, radius=1.0, centre=(0.1, -0.05, 0.2), distance=4.0, depth_tol=0.1, cos_min=0.5, power=2)
SPHERE_A = np.array([[0.30, -0.10, 0.05], [0.08, 0.25, -0.12], [-0.06, 0.10, 0.28]], f64)
SPHERE_B = np.array([0.5, 0.45, 0.4], f64)


def sphere_camera():
    """Anisotropic, off-centre: fx = 0.975 W, fy = 0.96 W, cx = W/2 - 3.25, cy = H/2 + 1.5 (the fusion sphere's)."""
    H, W = SPHERE["H"], SPHERE["W"]
    return np.array([[0.975 * W, 0, W / 2 - 3.25], [0, 0.96 * W, H / 2 + 1.5], [0, 0, 1]], f32)


def sphere_poses():
    """Ten look-at poses at distance 4 from the sphere's centre: a ring of eight at azimuth -180 + 45 k degrees, elevation -20 (even k) or
    +20 (odd k), then the top and the bottom (elevation -+89)."""
    views = [(-180.0 + 45.0 * k, -20.0 if k % 2 == 0 else 20.0) for k in range(8)] + [(0.0, -89.0), (0.0, 89.0)]
    return np.stack([pose_spherical(az, el, SPHERE["distance"], shift=SPHERE["centre"]) for az, el in views]).astype(f32)


def sphere_field(points):
    """float32 [n,3]: the linear colour field A x + b."""
    return (np.asarray(points, f64) @ SPHERE_A.T + SPHERE_B).astype(f32)


def sphere_mesh():
    """(verts, faces, analytic unit normals float32) of ``uv_sphere(12, 16)``."""
    s = SPHERE
    v, f = rast.uv_sphere(s["stacks"], s["slices"], s["radius"], s["centre"])
    n = v.astype(f64) - np.asarray(s["centre"])
    return v, f, (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)


def sphere_scene():
    """The quality scene: ``uv_sphere(12, 16)`` under ten 40 x 56 frames; the colours are the linear field rasterised as vertex attributes."""
    s = SPHERE
    verts, faces, normals = sphere_mesh()
    K, poses = sphere_camera(), sphere_poses()
    attrs = sphere_field(verts)
    frames = [raster_frame(verts, faces, dict(H=s["H"], W=s["W"], K=K, c2w=p), attrs) for p in poses]
    return _case("sphere", verts, np.stack([f[1] for f in frames]), np.stack([f[0] for f in frames]), cam_table(K, poses, len(poses)), normals,
                 depth_tol=s["depth_tol"], cos_min=s["cos_min"], power=s["power"], faces=faces)


def sphere_bound(verts, faces, normals, cams, depth_tol, cos_min, H, W):
    """The bound of DESIGN.md 3.26 on | baked colour - (A x + b) | (Euclidean over the channels), from the scene's own numbers:
    ``|A| (sqrt(2) t_max / min(fx, fy) (1 + slack) + depth_tol max|dir|)`` with ``slack = 1 / cos(acos(cos_min) + facet)``, ``facet`` the
    largest angle between a vertex normal and the normal of a face around it (faces without area aside).  Returns (bound, parts)."""
    verts, normals = np.asarray(verts, f64), np.asarray(normals, f64)
    cams = np.asarray(cams, f64)
    t_max, dir_max = 0.0, 0.0
    for cam in cams:
        c = cam[4:].reshape(3, 4)
        t_max = max(t_max, float((-((verts - c[:, 3]) @ c[:, :3])[:, 2]).max()))
        corners = np.array([((i - cam[2]) / cam[0], (j - cam[3]) / cam[1], 1.0) for i in (0, W - 1) for j in (0, H - 1)])
        dir_max = max(dir_max, float(np.linalg.norm(corners, axis=1).max()))
    tri = verts[np.asarray(faces, np.int64)]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(fn, axis=1)
    real = area > 1e-12 * area.max()
    fn = fn[real] / area[real, None]
    cosf = np.einsum("fcd,fd->fc", normals[np.asarray(faces, np.int64)[real]], fn)
    facet = float(np.arccos(np.clip(np.abs(cosf).min(), 0, 1)))                 # (whichever way the faces are wound)
    grazing = np.arccos(cos_min) + facet
    assert grazing < np.pi / 2, "the faces around an accepted vertex may be edge-on: no bound"
    slack = 1.0 / np.cos(grazing)
    norm_a = float(np.linalg.norm(SPHERE_A, 2))
    pixel = np.sqrt(2.0) * t_max / float(min(cams[:, 0].min(), cams[:, 1].min()))
    bound = norm_a * (pixel * (1.0 + slack) + depth_tol * dir_max)
    return bound, dict(norm_a=norm_a, t_max=t_max, pixel=pixel, facet_deg=float(np.rad2deg(facet)), slack=slack, dir_max=dir_max)


def path_faces(n):
    """int32 [n-1,3]: the degenerate faces (i, i, i + 1): ``vertex_adjacency`` makes i and i + 1 neighbours, so the mesh is a path graph."""
    i = np.arange(n - 1)
    return np.stack([i, i, i + 1], -1).astype(np.int32)


def fill_cases():
    """The hole-filling scenes (each a dict: name, colors [V,C], valid [V], faces): a path of 9 vertices with both ends baked; a sphere
    with a third of its vertices baked (several steps, vertices with two and more valid neighbours); and that sphere next to a second
    one with no baked vertex at all — an island that stays invalid."""
    ends = np.zeros((9, 2), f32)
    ends[0], ends[8] = (1.0, 8.0), (3.0, 16.0)
    valid = np.zeros(9, bool)
    valid[[0, 8]] = True
    out = [dict(name="path", colors=ends, valid=valid, faces=path_faces(9))]
    v, f = rast.uv_sphere(6, 8)
    rng = np.random.default_rng(2)
    colors = rng.uniform(0, 1, (len(v), 3)).astype(f32)
    valid = np.arange(len(v)) < len(v) // 3
    out.append(dict(name="sphere_cap", colors=colors, valid=valid, faces=f))
    out.append(dict(name="island", colors=np.concatenate([colors, colors]), valid=np.concatenate([valid, np.zeros(len(v), bool)]),
                    faces=np.concatenate([f, f + len(v)]).astype(np.int32), n_island=len(v)))
    return out


def catalogue():
    """The scenes the CPU and the GPU tests share (each a dict: name, verts, normals, images [n,H,W,C], depth [n,H,W], cams, depth_tol,
    cos_min, power, faces or None, and what the closed forms need)."""
    out = [exact_scene(), occlusion_scene(), depth_classes_scene()]
    out += [angle_scene(p) for p in (0, 1, 2, 8)]
    out += [best_tie_scene(), view_order_scene()]
    out.append(generic_scene("cams_per_view"))                                   # three views, three cameras; also the streaming scene
    out.append(generic_scene("cams_one", one_camera=True))                       # three views, one camera
    out += [generic_scene(f"channels_{C}", C=C, n_views=2, seed=20 + C) for C in (1, 3, 4, 16)]
    out.append(generic_scene("no_normals_16", C=16, n_views=2, seed=5))
    out[-1]["normals"] = None
    out += [generic_scene(f"vertices_{V}", V=V, n_views=2, seed=30 + V % 7) for V in (1, 255, 256, 257)]
    out += [bounds_scene(), smallest_frame_scene()]
    out.append(generic_scene("frame_8x12", H=8, W=12, n_views=2, seed=3))
    out.append(sphere_scene())
    return out
