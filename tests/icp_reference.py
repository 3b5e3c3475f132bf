"""NumPy restatement of the mesh registration (include/mofanerf_hip.h, mofa_icp_*; mofanerf_amd.mesh.transform_points /
fit_transform / register / register_meshes): the apply, the 36 terms of a correspondence for both metrics, the two-level sum, the border
flags and the reject rule, the trim rule, the Cholesky solve, the quaternion composition and the two loops, with the closest points taken
from dist_reference.brute_force.  Test code, not product.  ``mismatches`` is THE comparison of a result; tests/test_icp_reference_cpu.py
shows that every injected fault (``faults``: a set of the names in FAULTS) changes the result of a catalogue case."""
import math

import numpy as np

import dist_reference as dist

FAULTS = ("no_pivot", "cross_sign", "plane_no_scale", "keep_rejected", "border_wrong_edge", "trim_count", "compose_reversed", "dq_not_unit",
          "no_recentre", "flat_sum")
TERMS, CHUNK = 36, 1024
UNKNOWNS = {"translation": (3, 4, 5), "rigid": (0, 1, 2, 3, 4, 5), "similarity": (0, 1, 2, 3, 4, 5, 6)}
IDENTITY = (1.0, np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3))
widen = dist.widen


# ---- the device side --------------------------------------------------------------------------------------------------------------------
def apply(points, s, R, t):
    """out[i][r] = (float)(s ((R[r][0] x0 + R[r][1] x1) + R[r][2] x2) + t[r])"""
    x = widen(points).reshape(-1, 3)
    R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    with np.errstate(all="ignore"):
        cols = [np.float64(s) * ((R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1]) + R[r, 2] * x[:, 2]) + t[r] for r in range(3)]
        return np.stack(cols, -1).astype(np.float32)


def face_normals(verts, faces, face):
    """The unit normal of faces[face] as the kernel computes it, [N,3]; NaN rows where face is outside the mesh."""
    v, f = widen(verts).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face = np.asarray(face, dtype=np.int64)
    ok = (face >= 0) & (face < len(f))
    t = f[np.where(ok, face, 0)]
    n, _ = dist.zero_normal(v[t[:, 0]], v[t[:, 1]], v[t[:, 2]])
    with np.errstate(all="ignore"):
        n = n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    return np.where(ok[:, None], n, np.nan), ok


def terms(moved, target, weight, mu, metric, normals=None, face=None, verts=None, faces=None, faults=()):
    """[N,36] float64: A's upper triangle row by row, g, e of every correspondence; exact zeros where it is rejected."""
    y, c = widen(moved).reshape(-1, 3), widen(target).reshape(-1, 3)
    w = np.asarray(weight, dtype=np.float64).reshape(-1)
    mu = np.zeros(3) if "no_pivot" in faults else np.asarray(mu, dtype=np.float64)
    N = len(y)
    live = w > 0
    with np.errstate(all="ignore"):
        yh, d = y - mu, y - c
        zero, one = np.zeros(N), np.ones(N)
        sg = -1.0 if "cross_sign" in faults else 1.0
        if metric == "plane":
            if face is not None:
                n, ok = face_normals(verts, faces, face)
                live = live & ok
            else:
                n = widen(normals).reshape(-1, 3)
            J = [sg * (yh[:, 1] * n[:, 2] - yh[:, 2] * n[:, 1]), sg * (yh[:, 2] * n[:, 0] - yh[:, 0] * n[:, 2]),
                 sg * (yh[:, 0] * n[:, 1] - yh[:, 1] * n[:, 0]), n[:, 0], n[:, 1], n[:, 2],
                 zero if "plane_no_scale" in faults else (n[:, 0] * yh[:, 0] + n[:, 1] * yh[:, 1]) + n[:, 2] * yh[:, 2]]
            r = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
            cols = [w * (J[a] * J[b]) for a in range(7) for b in range(a, 7)] + [w * (J[a] * r) for a in range(7)] + [w * (r * r)]
        elif metric == "point":
            J = [[zero, sg * yh[:, 2], sg * -yh[:, 1], one, zero, zero, yh[:, 0]], [sg * -yh[:, 2], zero, sg * yh[:, 0], zero, one, zero, yh[:, 1]],
                 [sg * yh[:, 1], sg * -yh[:, 0], zero, zero, zero, one, yh[:, 2]]]
            cols = [w * ((J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b]) for a in range(7) for b in range(a, 7)]
            cols += [w * ((J[0][a] * d[:, 0] + J[1][a] * d[:, 1]) + J[2][a] * d[:, 2]) for a in range(7)]
            cols += [w * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])]
        else:
            raise ValueError(metric)
        out = np.stack(cols, -1)
    return out if "keep_rejected" in faults else np.where(live[:, None], out, 0.0)


def chunk_sums(rows):
    """One level of the sum: [M,c] -> [ceil(M / 1024), c]; thread t of a chunk adds its rows t, t + 256, t + 512, t + 768 to 0.0 in that order,
    then the tree w = 128 .. 1 runs over the 256 partial sums.  (Rows past M add nothing: a partial sum that starts at +0.0 is never -0.0.)"""
    rows = np.asarray(rows, dtype=np.float64)
    M, c = rows.shape
    n = (M + CHUNK - 1) // CHUNK
    pad = np.zeros((n * CHUNK, c))
    pad[:M] = rows
    a = pad.reshape(n, CHUNK // 256, 256, c)
    with np.errstate(all="ignore"):
        p = np.zeros((n, 256, c))
        for k in range(CHUNK // 256):
            p = p + a[:, k]
        w = 128
        while w >= 1:
            p[:, :w] = p[:, :w] + p[:, w:2 * w]
            w //= 2
    return p[:, 0]


def two_level(rows, faults=()):
    """The sum [c] of rows [M,c]: chunk_sums until one row is left (M = 0: zeros)."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.shape[0] == 0:
        return np.zeros(rows.shape[1])
    if "flat_sum" in faults:
        with np.errstate(all="ignore"):
            return np.cumsum(rows, 0)[-1]
    rows = chunk_sums(rows)
    while rows.shape[0] > 1:
        rows = chunk_sums(rows)
    return rows[0]


def border_flags(faces, V):
    """(face_border [F] uint8: bit k = the edge opposite corner k has one use over both directions; vert_border [V] uint8: the vertex is an
    end of such an edge).  An edge (a, a) is none."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    uses = {}
    for row in f:
        for k in range(3):
            a, b = int(row[(k + 1) % 3]), int(row[(k + 2) % 3])
            if a != b:
                uses[min(a, b), max(a, b)] = uses.get((min(a, b), max(a, b)), 0) + 1
    fb, vb = np.zeros(len(f), dtype=np.uint8), np.zeros(V, dtype=np.uint8)
    for i, row in enumerate(f):
        for k in range(3):
            a, b = int(row[(k + 1) % 3]), int(row[(k + 2) % 3])
            if a != b and uses[min(a, b), max(a, b)] == 1:
                fb[i] |= 1 << k
                vb[a] = vb[b] = 1
    return fb, vb


def reject(face, bary, faces, face_border, vert_border, faults=()):
    """[N] uint8: the border rule on closest_points' face / bary (exact comparisons with 0 on the float32 bary)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face, bary = np.asarray(face, dtype=np.int64), np.asarray(bary, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(face), dtype=np.uint8)
    for i in np.flatnonzero((face >= 0) & (face < len(f))):
        z = [bool(bary[i, k] == 0) for k in range(3)]
        shift = 1 if "border_wrong_edge" in faults else 0
        hit = any(z[k] and (face_border[face[i]] >> ((k + shift) % 3)) & 1 for k in range(3))
        if sum(z) == 2:
            hit = hit or bool(vert_border[f[face[i], z.index(False)]])
        out[i] = hit
    return out


def trim_keep(d2, valid, trim, faults=()):
    """valid & (d2 <= the ceil(trim n)-th smallest d2 among the n valid ones): ties are all kept."""
    valid = np.asarray(valid, dtype=bool)
    n = int(valid.sum())
    if trim is None or n == 0:
        return valid.copy()
    k = min(max(int(math.ceil(trim * n)), 1), n)
    if "trim_count" in faults:
        keep = np.zeros_like(valid)
        keep[np.flatnonzero(valid)[np.argsort(d2[valid], kind="stable")[:k]]] = True
        return keep
    return valid & (d2 <= np.sort(d2[valid])[k - 1])


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def solve(sums, unknowns):
    """x [7] of (sum A) x = -(sum g) over ``unknowns`` by the written Cholesky; None when singular."""
    sums = np.asarray(sums, dtype=np.float64)
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = sums[:28]
    H = np.where(np.tri(7, k=-1, dtype=bool), H.T, H)
    idx = list(unknowns)
    n = len(idx)
    A, rhs = H[np.ix_(idx, idx)], -sums[28:35][idx]
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0 and np.isfinite(s)):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        z = np.zeros(n)
        for i in range(n):
            s = rhs[i]
            for k in range(i):
                s = s - L[i, k] * z[k]
            z[i] = s / L[i, i]
        x = np.zeros(n)
        for i in reversed(range(n)):
            s = z[i]
            for k in range(i + 1, n):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    if not np.isfinite(x).all():
        return None
    full = np.zeros(7)
    full[idx] = x
    return full


def q_unit(q):
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def q_mul(a, b):
    return np.array([((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3], ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
                     ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1], ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0]])


def q_rotation(q):
    w, x, y, z = q
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def rotation_q(R):
    """Shepperd: the largest of the trace and the diagonal decides which component comes from the square root."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0:
        S = np.sqrt(tr + 1.0) * 2.0
        q = [0.25 * S, (R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        S = np.sqrt(((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2]) * 2.0
        q = [(R[2, 1] - R[1, 2]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[0, 2] + R[2, 0]) / S]
    elif R[1, 1] > R[2, 2]:
        S = np.sqrt(((1.0 + R[1, 1]) - R[0, 0]) - R[2, 2]) * 2.0
        q = [(R[0, 2] - R[2, 0]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S]
    else:
        S = np.sqrt(((1.0 + R[2, 2]) - R[0, 0]) - R[1, 1]) * 2.0
        q = [(R[1, 0] - R[0, 1]) / S, (R[0, 2] + R[2, 0]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S]
    return q_unit(np.array(q))


def compose(state, x, mu, faults=()):
    """(s, q, t) after the step x about mu: s <- ds s, q <- unit(dq (x) q), t <- ds dR (t - mu) + mu + tau; None when ds <= 0."""
    s, q, t = state
    mu = np.asarray(mu, dtype=np.float64)
    ds = 1.0 + x[6]
    if not ds > 0:
        return None
    dq = np.array([1.0, 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]])
    if "dq_not_unit" not in faults:
        dq = q_unit(dq)
    dR = q_rotation(dq)
    u = t if "no_recentre" in faults else t - mu
    v = np.array([(dR[r, 0] * u[0] + dR[r, 1] * u[1]) + dR[r, 2] * u[2] for r in range(3)])
    t = (ds * v + x[3:6]) if "no_recentre" in faults else ((ds * v + mu) + x[3:6])
    return ds * s, q_unit(q_mul(q, dq) if "compose_reversed" in faults else q_mul(dq, q)), t


def step_size(x, extent):
    return float(max(np.abs(x[:3]).max(), np.abs(x[3:6]).max() / extent, abs(x[6])))


def box_of(points):
    """(centre [3], largest edge or 1) of the float32 points, in fp64."""
    p = widen(points).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    e = float((hi - lo).max())
    return (lo + hi) * 0.5, e if e > 0 else 1.0


def init_state(init):
    if init is None:
        return IDENTITY
    if isinstance(init, dict):
        s, R, t = float(init["scale"]), np.asarray(init["rotation"], dtype=np.float64), np.asarray(init["translation"], dtype=np.float64)
    else:
        M = np.asarray(init, dtype=np.float64).reshape(4, 4)
        s = float(np.sqrt((M[0, 0] * M[0, 0] + M[0, 1] * M[0, 1]) + M[0, 2] * M[0, 2]))
        R, t = M[:3, :3] / s, M[:3, 3]
    return s, rotation_q(R), t.copy()


def result(state, moved, history, iterations, status):
    s, q, t = state
    R = q_rotation(q)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return {"scale": float(s), "rotation": R, "translation": np.asarray(t, dtype=np.float64).copy(), "matrix": M, "moved": moved,
            "history": history, "iterations": iterations, "status": status}


def _update(state, sums, wsum, model, mu, extent, entry, faults):
    with np.errstate(all="ignore"):
        entry["rms"] = float(np.sqrt(sums[35] / wsum)) if wsum > 0 else float("nan")
    entry["step"] = float("nan")
    if entry["used"] == 0:
        return None, "no_correspondences"
    x = solve(sums, UNKNOWNS[model])
    new = None if x is None else compose(state, x, mu, faults)
    if new is None:
        return None, "singular"
    entry["step"] = step_size(x, extent)
    return new, None


def fit_transform(src, dst, weight=None, normals=None, model="rigid", metric="point", iterations=8, init=None, tol=0.0, faults=()):
    src, dst = np.asarray(src, dtype=np.float32).reshape(-1, 3), np.asarray(dst, dtype=np.float32).reshape(-1, 3)
    N = len(src)
    weight = np.ones(N) if weight is None else np.asarray(weight, dtype=np.float64)
    state = init_state(init)
    if N == 0:
        return result(state, src.copy(), [], 0, "empty")
    finite = np.isfinite(dst).all(1)
    mu, extent = box_of(dst[finite]) if finite.any() else (np.zeros(3), 1.0)
    history, status, done = [], "iterations", 0
    for _ in range(iterations):
        moved = apply(src, state[0], q_rotation(state[1]), state[2])
        ok = finite & np.isfinite(moved).all(1)
        w = weight if "keep_rejected" in faults else np.where(ok, weight, 0.0)
        entry = {"used": int((np.where(ok, weight, 0.0) > 0).sum()), "rejected": {"non_finite": int((~ok).sum())}}
        history.append(entry)
        sums = two_level(terms(moved, dst, w, mu, metric, normals=normals, faults=faults), faults)
        new, stop = _update(state, sums, two_level(w[:, None], faults)[0], model, mu, extent, entry, faults)
        if stop:
            status = stop
            break
        state, done = new, done + 1
        if entry["step"] <= tol:
            status = "converged"
            break
    return result(state, apply(src, state[0], q_rotation(state[1]), state[2]), history, done, status)


def register(points, verts, faces, model="rigid", metric="plane", iterations=30, init=None, weight=None, max_distance=None, trim=None,
             reject_border=True, tol=0.0, pivot=None, faults=()):
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    verts, faces = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    N = len(points)
    weight = np.ones(N) if weight is None else np.asarray(weight, dtype=np.float64)
    state = init_state(init)
    if N == 0:
        return result(state, points.copy(), [], 0, "empty")
    if len(verts) == 0 or len(faces) == 0:
        return result(state, apply(points, state[0], q_rotation(state[1]), state[2]), [], 0, "no_correspondences")
    mu, extent = box_of(verts)
    mu = mu if pivot is None else np.asarray(pivot, dtype=np.float64)
    fb, vb = border_flags(faces, len(verts))
    history, status, done = [], "iterations", 0
    for _ in range(iterations):
        moved = apply(points, state[0], q_rotation(state[1]), state[2])
        res = dist.brute_force(moved, verts, faces, np.inf if max_distance is None else float(max_distance))
        finite = np.isfinite(moved).all(1) & (np.isfinite(res["d2"]) | (res["face"] < 0))
        has = finite & (res["face"] >= 0)
        on_border = has & (reject(res["face"], res["bary"], faces, fb, vb, faults) != 0) if reject_border else np.zeros(N, dtype=bool)
        valid = has & ~on_border & (weight > 0)
        keep = trim_keep(res["d2"], valid, trim, faults)
        w = weight if "keep_rejected" in faults else np.where(keep, weight, 0.0)
        entry = {"used": int(keep.sum()), "rejected": {"non_finite": int((~finite).sum()),
                                                       "beyond" if max_distance is not None else "no_face": int((finite & ~has).sum()),
                                                       "border": int(on_border.sum()), "trimmed": int(valid.sum()) - int(keep.sum())}}
        history.append(entry)
        sums = two_level(terms(moved, res["closest"], w, mu, metric, face=res["face"], verts=verts, faces=faces, faults=faults), faults)
        new, stop = _update(state, sums, two_level(w[:, None], faults)[0], model, mu, extent, entry, faults)
        if stop:
            status = stop
            break
        state, done = new, done + 1
        if entry["step"] <= tol:
            status = "converged"
            break
    return result(state, apply(points, state[0], q_rotation(state[1]), state[2]), history, done, status)


def register_meshes(verts_a, faces_a, verts_b, faces_b, spacing, **kw):
    pts, _, weight, _, _ = dist.sample_faces(verts_a, faces_a, spacing)
    va = np.asarray(verts_a, dtype=np.float32).reshape(-1, 3)
    out = register(np.concatenate([pts, va]), verts_b, faces_b, weight=np.concatenate([weight, np.zeros(len(va))]), **kw)
    out["verts"], out["n_samples"] = out["moved"][len(pts):], len(pts)
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def mismatches(got, want):
    """The parts of a result (of mesh.fit_transform / register with ``moved`` on the host, or of the restatement) that differ from ``want`` in
    any bit: scale, rotation, translation, matrix, moved, status, iterations and every history entry."""
    bad = [k for k in ("scale", "rotation", "translation", "matrix") if not _bits(got[k], want[k])]
    if np.asarray(got["moved"]).dtype != np.float32 or not dist._same(np.asarray(got["moved"]), np.asarray(want["moved"])):
        bad.append("moved")
    bad += [k for k in ("status", "iterations") if got[k] != want[k]]
    if len(got["history"]) != len(want["history"]):
        return bad + ["history length"]
    for i, (g, w) in enumerate(zip(got["history"], want["history"])):
        if g["used"] != w["used"] or g["rejected"] != w["rejected"] or not _bits(g["rms"], w["rms"]) or not _bits(g["step"], w["step"]):
            bad.append(f"history[{i}]")
    return bad


# ---- the scene catalogue ----------------------------------------------------------------------------------------------------------------
AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
OFFSET = np.array([0.02, -0.015, 0.01])
TRANSFORMS = (("rigid5", 5.0, 1.0), ("rigid10", 10.0, 1.0), ("rigid20", 20.0, 1.0), ("similarity10", 10.0, 1.1))
_cache = {}


def patch():
    """The face patch: a 17 x 17 height field on [-1, 1]^2, 289 vertices, 512 faces (float32, int32)."""
    if "patch" not in _cache:
        g = np.linspace(-1.0, 1.0, 17)
        x, y = np.meshgrid(g, g, indexing="ij")
        z = (0.6 * np.exp(-((x - 0.1) ** 2 + (y + 0.2) ** 2) / 0.15) + 0.25 * np.exp(-((x + 0.45) ** 2 + (y - 0.35) ** 2) / 0.05)
             - 0.2 * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.08) + 0.1 * x * y + 0.15 * x)
        verts = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
        i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        v00 = (i * 17 + j).reshape(-1)
        v10, v01, v11 = v00 + 17, v00 + 1, v00 + 18
        _cache["patch"] = (verts, np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32))
    return _cache["patch"]


def crop():
    """The patch's faces with centroid x < 0.4 (all 289 vertices stay)."""
    verts, faces = patch()
    return verts, faces[widen(verts)[faces.astype(np.int64)].mean(1)[:, 0] < 0.4].copy()


def cube():
    """The unit cube of the other references (wind_reference.cube): 8 vertices, 12 faces, outward normals."""
    import wind_reference
    return wind_reference.cube()


def flat_square():
    return dist.square(4)


def samples(limit):
    """The quadrature of the patch at spacing 0.15 restricted to |x|, |y| < limit: (points float32, weight float64)."""
    if ("samples", limit) not in _cache:
        pts, _, weight, _, _ = dist.sample_faces(*patch(), 0.15)
        keep = (np.abs(pts[:, 0]) < limit) & (np.abs(pts[:, 1]) < limit)
        _cache["samples", limit] = (pts[keep].copy(), weight[keep].copy())
    return _cache["samples", limit]


def known_transform(angle_deg, scale):
    """(s, R, t): a rotation by ``angle_deg`` about AXIS through the origin, the scale and OFFSET (Rodrigues; test data, not the product's path)."""
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -AXIS[2], AXIS[1]], [AXIS[2], 0, -AXIS[0]], [-AXIS[1], AXIS[0], 0]])
    return float(scale), np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K), OFFSET.copy()


def displaced(points, angle_deg, scale):
    """``points`` moved by the inverse of known_transform, float32: registration has to bring them back onto ``points``."""
    s, R, t = known_transform(angle_deg, scale)
    return (((widen(points) - t) @ R) / s).astype(np.float32)


def source(name, limit=0.8):
    """(the displaced source points, the truth they should return to, their weights) of one of TRANSFORMS."""
    _, angle, scale = next(t for t in TRANSFORMS if t[0] == name)
    pts, weight = samples(limit)
    return displaced(pts, angle, scale), pts, weight
