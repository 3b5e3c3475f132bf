"""Yardsticks of the UV texture baking (``mofa_uv_*``, ``mesh.uv_locate`` / ``texel_map`` / ``texel_surface`` / ``texture_image`` /
``dilate_texture`` / ``sample_texture`` / ``face_atlas``).

* :func:`locate`, :func:`surface`, :func:`dilate_step` and :func:`sample` restate the four kernels in NumPy, operation for operation, in
  ``np.float64`` on the float32 inputs widened — the GPU results must equal them bit for bit, the counters integer for integer.  ``fault``
  injects one mistake (``FAULTS``) so that tests/test_uv_reference_cpu.py can show that the comparison catches it.
* :func:`texel_map`, :func:`texel_surface`, :func:`texture_image` (on top of tests/bake_reference.py) and :func:`face_atlas` stand for the
  ``mesh`` calls of the same names.
* :func:`catalogue` lists the UV layouts the CPU and the GPU tests share.
"""
import math

import numpy as np

import bake_reference as br
import icp_reference as icp
import raster_reference as rast
from raster_reference import same_bits  # noqa: F401  (re-exported for the tests)

f32, f64 = np.float32, np.float64
FAULTS = ("index_order_edges", "strict_inside", "highest_face", "no_v_flip", "corner_centre", "reject_mirrored", "dilate_in_place", "dilate_4",
          "wrap", "wrong_corner", "swap_uv")
COUNTS = ("degenerate", "non_finite_queries", "face_tests", "multi")
GRID_AUTO_CAP = 256


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def texture_size(size):
    s = np.asarray(size).reshape(-1)
    return (int(s[0]), int(s[0])) if s.size == 1 else (int(s[0]), int(s[1]))


def centres(size, fault=None):
    """float64 [Ht Wt, 2]: (u, v) of the texel centres, row-major."""
    Ht, Wt = texture_size(size)
    half = 0.0 if fault == "corner_centre" else 0.5
    u = (np.arange(Wt, dtype=f64) + half) / f64(Wt)
    v = (np.arange(Ht, dtype=f64) + half) / f64(Ht)
    if fault != "no_v_flip":
        v = 1.0 - v
    return np.stack([np.broadcast_to(u[None, :], (Ht, Wt)), np.broadcast_to(v[:, None], (Ht, Wt))], -1).reshape(-1, 2).copy()


def default_grid(F):
    g = int(min(max(math.ceil(math.sqrt(max(int(F), 0) / 4.0)), 1), GRID_AUTO_CAP))
    return (g, g)


def grid_of(grid, F):
    if grid is None:
        return default_grid(F)
    g = np.asarray(grid).reshape(-1)
    return (int(g[0]), int(g[0])) if g.size == 1 else (int(g[0]), int(g[1]))


def grid_spec(uv, grid):
    """(origin [2], cell [2]) of the grid over the box of the float32 UVs: cell = extent / n, 1 on a side of no extent."""
    lo, hi = uv.min(0), uv.max(0)
    extent = hi - lo
    return lo, np.where(extent > 0, extent / np.asarray(grid, f64), 1.0)


def cell_index(x, origin, cell, n):
    with np.errstate(all="ignore"):
        t = np.floor((np.asarray(x, f64) - origin) / cell)
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, 0, n - 1).astype(np.int64)


def _edge(X, Y, q, mirrored, fault):
    """e of the edge the face runs from X to Y, evaluated on the edge's endpoints in coordinate order."""
    from_q = (Y[0] < X[0]) or (Y[0] == X[0] and Y[1] < X[1])
    if fault == "index_order_edges":
        from_q = False
    P, Q = (Y, X) if from_q else (X, Y)
    e = (Q[0] - P[0]) * (q[:, 1] - P[1]) - (Q[1] - P[1]) * (q[:, 0] - P[0])
    return -e if from_q != mirrored else e


def locate(queries, uvs, uv_faces, grid=None, fault=None):
    """dict of ``mofa_uv_locate`` / ``mesh.uv_locate``: ``face`` int32 [N], ``bary`` float64 [N,3], ``counts``, ``grid``."""
    assert fault is None or fault in FAULTS
    q = np.asarray(queries, f64).reshape(-1, 2)
    uv = np.asarray(uvs, f32).reshape(-1, 2).astype(f64)
    if fault == "swap_uv":
        q = q[:, ::-1]
    tf = np.asarray(uv_faces, np.int64).reshape(-1, 3)
    N, F = len(q), len(tf)
    face, bary = np.full(N, -1, np.int32), np.full((N, 3), np.nan, f64)
    finite = np.isfinite(q).all(1)
    counts = dict.fromkeys(COUNTS, 0)
    counts["non_finite_queries"] = int((~finite).sum())
    if N == 0 or F == 0 or len(uv) == 0:
        return {"face": face, "bary": bary, "counts": counts, "grid": grid_of(grid, 0) if grid is not None else (1, 1)}
    grid = grid_of(grid, F)
    origin, cell = grid_spec(uv, grid)
    cq = [cell_index(q[:, a], origin[a], cell[a], grid[a]) for a in (0, 1)]
    strict = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for f in range(F):
            A, B, Cc = uv[tf[f]]
            D = (B[0] - A[0]) * (Cc[1] - A[1]) - (B[1] - A[1]) * (Cc[0] - A[0])
            degenerate = (not np.isfinite(D)) or D == 0
            counts["degenerate"] += int(degenerate)
            mn, mx = uv[tf[f]].min(0), uv[tf[f]].max(0)
            if mn[0] == mx[0] or mn[1] == mx[1]:                                  # flat: the binning lists it nowhere
                continue
            lo = [cell_index(mn[a], origin[a], cell[a], grid[a]) for a in (0, 1)]
            hi = [cell_index(mx[a], origin[a], cell[a], grid[a]) for a in (0, 1)]
            listed = finite & (cq[0] >= lo[0]) & (cq[0] <= hi[0]) & (cq[1] >= lo[1]) & (cq[1] <= hi[1])
            counts["face_tests"] += int(listed.sum())
            if degenerate or (fault == "reject_mirrored" and D < 0):
                continue
            mirrored = bool(D < 0)
            e = [_edge(B, Cc, q, mirrored, fault), _edge(Cc, A, q, mirrored, fault), _edge(A, B, q, mirrored, fault)]
            S = (e[0] + e[1]) + e[2]
            all_strict = (e[0] > 0) & (e[1] > 0) & (e[2] > 0)
            inside = all_strict if fault == "strict_inside" else ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0))
            inside = listed & inside & (S > 0)
            strict += (listed & all_strict & (S > 0)).astype(np.int64)
            take = inside if fault == "highest_face" else (inside & (face < 0))
            for k in range(3):
                bary[take, k] = (e[(k + 1) % 3] if fault == "wrong_corner" else e[k])[take] / S[take]
            face[take] = f
    counts["multi"] = int((strict >= 2).sum())
    return {"face": face, "bary": bary, "counts": counts, "grid": grid}


def texel_map(uvs, uv_faces, size, grid=None, fault=None):
    """dict of ``mesh.texel_map``."""
    Ht, Wt = texture_size(size)
    F = len(np.asarray(uv_faces).reshape(-1, 3))
    out = locate(centres((Ht, Wt), fault), uvs, uv_faces, grid, fault)
    covered = out["face"] >= 0
    index = np.flatnonzero(covered).astype(np.int64)
    counts = {"covered": int(covered.sum()), "multi": out["counts"]["multi"], "degenerate": out["counts"]["degenerate"],
              "faces_without_texels": F - len(np.unique(out["face"][covered])), "face_tests": out["counts"]["face_tests"]}
    return {"face": out["face"].reshape(Ht, Wt), "bary": out["bary"].reshape(Ht, Wt, 3), "covered": covered.reshape(Ht, Wt), "index": index,
            "counts": counts, "size": (Ht, Wt), "grid": out["grid"], "n_faces": F}


def surface(face, bary, verts, faces, normals=None):
    """(points float32 [N,3], normals float32 [N,3]) of ``mofa_uv_surface`` for valid faces."""
    x = np.asarray(verts, f32).astype(f64)
    tri = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    b = np.asarray(bary, f64)
    X = [x[tri[:, k]] for k in range(3)]
    with np.errstate(all="ignore"):
        points = ((b[:, 0:1] * X[0] + b[:, 1:2] * X[1]) + b[:, 2:3] * X[2]).astype(f32)
        if normals is not None:
            n = np.asarray(normals, f32).astype(f64)
            m = (b[:, 0:1] * n[tri[:, 0]] + b[:, 1:2] * n[tri[:, 1]]) + b[:, 2:3] * n[tri[:, 2]]
        else:
            p, r = X[1] - X[0], X[2] - X[0]
            m = np.stack([p[:, 1] * r[:, 2] - p[:, 2] * r[:, 1], p[:, 2] * r[:, 0] - p[:, 0] * r[:, 2], p[:, 0] * r[:, 1] - p[:, 1] * r[:, 0]], -1)
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = (length > 0) & np.isfinite(length)
        unit = np.where(ok[:, None], (m / length[:, None]).astype(f32), f32(0))
    return points, unit.astype(f32)


def texel_surface(tmap, verts, faces, normals=None):
    index = tmap["index"]
    return surface(tmap["face"].reshape(-1)[index], tmap["bary"].reshape(-1, 3)[index], verts, faces, normals)


def dilate_step(texture, valid, fault=None):
    """One step of ``mofa_uv_dilate``: (texture float32 [Ht,Wt,C], valid bool [Ht,Wt]) from the INPUT arrays."""
    Ht, Wt, C = texture.shape
    src_t, src_v = texture, valid
    out_t, out_v = texture.copy(), valid.copy()
    if fault == "dilate_in_place":
        src_t, src_v = out_t, out_v
    for i in range(Ht):
        for j in range(Wt):
            if valid[i, j]:
                continue
            s, k = np.zeros(C, f64), 0
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (di == 0 and dj == 0) or (fault == "dilate_4" and di != 0 and dj != 0):
                        continue
                    a, b = i + di, j + dj
                    if 0 <= a < Ht and 0 <= b < Wt and src_v[a, b]:
                        s = s + src_t[a, b].astype(f64)
                        k += 1
            if k:
                out_t[i, j] = (s / f64(k)).astype(f32)
                out_v[i, j] = True
    return out_t, out_v


def dilate(texture, valid, iterations, fault=None):
    """(texture, valid, remaining) of ``mesh.dilate_texture``."""
    texture, valid = np.asarray(texture, f32).copy(), np.asarray(valid, bool).copy()
    for _ in range(iterations):
        texture, valid = dilate_step(texture, valid, fault)
    return texture, valid, int((~valid).sum())


def texture_image(state, tmap, blend="mean", fill=0.0, dilate_steps=0, fault=None):
    """dict of ``mesh.texture_image`` from a restated baking state (tests/bake_reference.py) over the covered texels."""
    Ht, Wt = tmap["size"]
    baked = br.resolve(state, blend, fill)
    C = baked["colors"].shape[1]
    texture, valid = np.full((Ht * Wt, C), f32(fill), f32), np.zeros(Ht * Wt, bool)
    texture[tmap["index"]], valid[tmap["index"]] = baked["colors"], baked["valid"]
    texture, valid, remaining = dilate(texture.reshape(Ht, Wt, C), valid.reshape(Ht, Wt), dilate_steps, fault)
    return {"texture": texture, "valid": valid, "counts": baked["counts"], "remaining": remaining}


def sample(texture, face, bary, uvs, uv_faces, background=0.0, fault=None):
    """float32 [H,W,C] of ``mofa_uv_sample`` / ``mesh.sample_texture``."""
    tex = np.asarray(texture, f32)
    Ht, Wt, C = tex.shape
    face = np.asarray(face, np.int64)
    H, W = face.shape
    uv = np.asarray(uvs, f32).astype(f64)
    tf = np.asarray(uv_faces, np.int64)
    hit = (face >= 0) & (face < len(tf))
    tri = tf[np.where(hit, face, 0)]
    b = np.asarray(bary, f32).astype(f64)
    with np.errstate(all="ignore"):
        u = (b[..., 0] * uv[tri[..., 0], 0] + b[..., 1] * uv[tri[..., 1], 0]) + b[..., 2] * uv[tri[..., 2], 0]
        v = (b[..., 0] * uv[tri[..., 0], 1] + b[..., 1] * uv[tri[..., 1], 1]) + b[..., 2] * uv[tri[..., 2], 1]
        if fault == "swap_uv":
            u, v = v, u
        hit = hit & np.isfinite(u) & np.isfinite(v)
        u, v = np.where(hit, u, 0.5), np.where(hit, v, 0.5)
        x = u * f64(Wt) - 0.5
        y = (v * f64(Ht) - 0.5) if fault == "no_v_flip" else ((1.0 - v) * f64(Ht) - 0.5)
        if fault == "corner_centre":
            x, y = u * f64(Wt), (1.0 - v) * f64(Ht)
        xf, yf = np.floor(x), np.floor(y)
        fx, fy = x - xf, y - yf
        if fault == "wrap":
            pick = lambda t, n: np.mod(t, n).astype(np.int64)
        else:
            pick = lambda t, n: np.clip(t, 0, n - 1).astype(np.int64)
        j0, j1, i0, i1 = pick(xf, Wt), pick(xf + 1.0, Wt), pick(yf, Ht), pick(yf + 1.0, Ht)
        c00, c10, c01, c11 = (tex[i, j].astype(f64) for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
        a = c00 + fx[..., None] * (c10 - c00)
        bb = c01 + fx[..., None] * (c11 - c01)
        col = (a + fy[..., None] * (bb - a)).astype(f32)
    return np.where(hit[..., None], col, f32(background)).astype(f32)


def face_atlas(n_faces, size, padding=1.0):
    """(uvs float32 [3 F,2], uv_faces int32 [F,3], info) of ``mesh.face_atlas``, face by face; ``ValueError`` where it refuses."""
    Ht, Wt = texture_size(size)
    F, p = int(n_faces), float(padding)
    n = 1
    while 2 * n * n < F:
        n += 1
    h, w = Ht / n, Wt / n
    d = p * math.sqrt(1.0 / (w * w) + 1.0 / (h * h))
    if not (w * (1.0 - d - p / h) - p >= 1.0 and h * (1.0 - d - p / w) - p >= 1.0):
        raise ValueError(f"cells of {h} x {w} texels are too small; size {n * int(math.ceil(1.0 + (2.0 + math.sqrt(2.0)) * p))} would do")
    xy = []
    for f in range(F):
        k = f // 2
        x0, y0 = (k % n) * w, (k // n) * h
        if f % 2 == 0:                                                            # toward the cell's top-left corner
            xy += [(x0 + p, y0 + p), (x0 + p, y0 + h * (1.0 - d - p / w)), (x0 + w * (1.0 - d - p / h), y0 + p)]
        else:                                                                     # toward its bottom-right corner
            xy += [(x0 + w - p, y0 + h - p), (x0 + w - p, y0 + h * (d + p / w)), (x0 + w * (d + p / h), y0 + h - p)]
    xy = np.asarray(xy, f64).reshape(-1, 2)
    uvs = np.stack([xy[:, 0] / Wt, 1.0 - xy[:, 1] / Ht], -1).astype(f32)
    return uvs, np.arange(3 * F, dtype=np.int32).reshape(F, 3), {"n": n, "cell": (h, w), "padding": p, "size": (Ht, Wt)}


# ---- the layouts -----------------------------------------------------------------------------------------------------------------------
def _layout(name, uvs, uv_faces, sizes, verts=None, faces=None, normals=None, **extra):
    uvs = np.ascontiguousarray(uvs, f32).reshape(-1, 2)
    uv_faces = np.ascontiguousarray(uv_faces, np.int32).reshape(-1, 3)
    if verts is None:                                                             # a surface of its own: the UVs lifted off the plane
        u, v = uvs[:, 0].astype(f64), uvs[:, 1].astype(f64)
        verts, faces = np.stack([u, v, 0.3 * u - 0.2 * v + 0.1 * u * v], -1), uv_faces
    return dict(name=name, uvs=uvs, uv_faces=uv_faces, sizes=[texture_size(s) for s in sizes], verts=np.ascontiguousarray(verts, f32).reshape(-1, 3),
                faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), normals=None if normals is None else np.ascontiguousarray(normals, f32),
                **extra)


QUAD_UV = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], f64)
QUAD_FACES = np.array([(0, 1, 2), (0, 2, 3)], np.int32)                            # cut along (0, 0) - (1, 1)


def quad():
    """The unit square cut along (0,0)-(1,1), uvs = xy: at 4 x 4 the centres with i + j = 3 lie exactly on the shared diagonal."""
    return _layout("quad", QUAD_UV, QUAD_FACES, [(4, 4), (5, 3)], verts=np.concatenate([QUAD_UV, np.zeros((4, 1))], 1), faces=QUAD_FACES)


def sphere_layout(stacks=12, slices=16):
    """(uvs float32 [(stacks+1)(slices+1),2], uv_faces): latitude-longitude for ``uv_sphere(stacks, slices)``: u = b / slices with the
    seam column b = slices duplicated (T > V), v = 1 - a / stacks; face order and corner order are ``uv_sphere``'s."""
    a, b = np.meshgrid(np.arange(stacks + 1), np.arange(slices + 1), indexing="ij")
    uvs = np.stack([b / slices, 1.0 - a / stacks], -1).reshape(-1, 2)
    faces = []
    for i in range(stacks):
        for j in range(slices):
            p, q, r, s = i * (slices + 1) + j, i * (slices + 1) + j + 1, (i + 1) * (slices + 1) + j, (i + 1) * (slices + 1) + j + 1
            faces += [(p, r, q), (q, r, s)]
    return uvs.astype(f32), np.asarray(faces, np.int32)


def sphere():
    verts, faces, normals = br.sphere_mesh()
    uvs, uv_faces = sphere_layout(br.SPHERE["stacks"], br.SPHERE["slices"])
    assert len(uvs) > len(verts) and len(uv_faces) == len(faces)
    return _layout("sphere", uvs, uv_faces, [(16, 32), (64, 128)], verts=verts, faces=faces, normals=normals)


def octahedron():
    verts = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)
    faces = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int32)
    return verts, faces


def patch13():
    """The 13 x 13 corner of tests/icp_reference.py's height-field patch: its 289 vertices, the 288 faces among the first 13 x 13."""
    verts, faces = icp.patch()
    keep = ((faces // 17 < 13) & (faces % 17 < 13)).all(1)
    return verts, np.ascontiguousarray(faces[keep])


def catalogue():
    """The UV layouts the CPU and the GPU tests share (each a dict: name, uvs, uv_faces, sizes, verts, faces, normals or None)."""
    out = [quad(), sphere()]
    out.append(_layout("mirrored", np.stack([1.0 - QUAD_UV[:, 0], QUAD_UV[:, 1]], -1) * 0.75 + 0.125, QUAD_FACES, [(8, 8), (7, 5)]))
    out.append(_layout("overlap", np.concatenate([QUAD_UV * 0.8 + 0.1, QUAD_UV * 0.8 + 0.1]), np.concatenate([QUAD_FACES, QUAD_FACES + 4]),
                       [(8, 8), (5, 9)]))
    out.append(_layout("degenerate", [(0, 0), (1, 0), (0, 1), (0, 0), (0.5, 0.5), (1, 1), (1, 1), (1, 1), (1, 0.25)], [(0, 1, 2), (3, 4, 5), (6, 7, 8)],
                       [(8, 8), (6, 10)]))
    out.append(_layout("outside", QUAD_UV * 2.0 - 0.5, QUAD_FACES, [(8, 8), (5, 7)]))
    out.append(_layout("sliver", [(0, 0), (1, 0), (0, 0.4), (0.1, 0.52), (0.9, 0.53), (0.5, 0.528)], [(0, 1, 2), (3, 4, 5)], [(8, 8)]))
    for name, (verts, faces), size in (("atlas_octahedron", octahedron(), (16, 16)), ("atlas_patch", patch13(), (64, 64))):
        uvs, uv_faces, info = face_atlas(len(faces), size)
        out.append(_layout(name, uvs, uv_faces, [size], verts=verts, faces=faces, info=info))
    return out


def random_queries(layout, n=1000, seed=0):
    """float64 [n,2]: seeded queries over [-0.6, 1.6]^2 — most of them uniform, then NaN and infinities, points ON vertices, points on
    edges (midpoints and other exact binary fractions of an edge) and face centroids."""
    rng = np.random.default_rng(seed + len(layout["uvs"]))
    uv = layout["uvs"].astype(f64)
    tf = layout["uv_faces"].astype(np.int64)
    q = rng.uniform(-0.1, 1.1, (n, 2))
    q[: n // 8] = rng.uniform(-0.6, 1.6, (n // 8, 2))
    k = n // 8
    q[k:k + 4] = [(np.nan, 0.5), (0.5, np.inf), (-np.inf, np.nan), (np.nan, np.nan)]
    k += 4
    m = min(n // 8, len(uv))
    q[k:k + m] = uv[rng.integers(0, len(uv), m)]
    k += m
    for frac in (0.5, 0.25, 0.75):
        f = rng.integers(0, len(tf), n // 16)
        c = rng.integers(0, 3, n // 16)
        a, b = uv[tf[f, c]], uv[tf[f, (c + 1) % 3]]
        q[k:k + n // 16] = a + frac * (b - a)
        k += n // 16
    f = rng.integers(0, len(tf), n // 16)
    q[k:k + n // 16] = (uv[tf[f, 0]] + uv[tf[f, 1]] + uv[tf[f, 2]]) / 3.0
    return np.ascontiguousarray(q)


# ---- the sphere scene's quality ----------------------------------------------------------------------------------------------------------
def wave_field(points, period=0.5):
    """float32 [n,3]: the colour field 0.5 + 0.5 sin(2 pi x_k / period) per channel."""
    return (0.5 + 0.5 * np.sin(2.0 * np.pi * np.asarray(points, f64) / period)).astype(f32)


def interior_bound(verts, faces, normals, cams, depth_tol, cos_min, H, W):
    """The bound of DESIGN.md 3.27 on | baked colour - (A x + b) | at a face-INTERIOR point whose normal is the normalised barycentric
    interpolation of the vertex normals.  It is 3.26's argument re-derived for such a point: the footprint of a view is bilinear between
    four pixels, each a point of the mesh within ``sqrt(2) t_max / min(fx, fy)`` of the pixel's ray at the texel's depth, stretched along
    the surface by ``1 / cos`` of the angle between the view and the FACE the pixel hits, and off in depth by at most ``depth_tol`` along
    a ray of length factor ``max|dir|``.  The one change is the angle: the interpolated normal of an interior point lies in the cone of
    its face's three vertex normals, so it is within ``facet`` of the face's normal where ``facet`` is the largest angle between a vertex
    normal and the normal of a face around it — the same number as for a vertex, because a convex combination of three directions each
    within ``facet`` of the face normal stays within ``facet`` of it.  Hence the same formula, evaluated with ``t_max`` over the mesh's
    vertices (a face's points are no farther than its farthest corner).  Returns (bound, parts)."""
    return br.sphere_bound(verts, faces, normals, cams, depth_tol, cos_min, H, W)
