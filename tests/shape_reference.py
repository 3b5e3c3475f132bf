"""NumPy restatement of the linear shape model (include/mofanerf_hip.h, mofa_shape_*; mofanerf_amd.mesh.shape_model /
shape_synthesize / shape_project / shape_fit): the weighted Gram matrix with its two-level sum, the centring, the combination, the plane
rows, the cyclic Jacobi, the Cholesky solve and the three public calls, the last with the closest points of dist_reference.brute_force and
the pose step and the rejection of icp_reference.  Test code, not product.  ``mismatches`` is THE comparison of a result;
tests/test_shape_reference_cpu.py shows that every injected fault (``faults``: a set of the names in FAULTS) changes a result."""
import math

import numpy as np

import dist_reference as dist
import icp_reference as icp

FAULTS = ("chunk_reversed", "weight_first", "group_ignored", "keep_rejected", "flat_sum", "m_not_m1", "unsorted", "no_sign_rule", "no_lambda_c",
          "normal_not_rotated", "kept_border")
MAX_ROWS, JACOBI_SWEEPS = 256, 64
PIVOT_FLOOR = 2.0 ** -40      # a pivot below this share of its diagonal entry has lost 40 bits to cancellation: singular
widen = dist.widen


# ---- the device side --------------------------------------------------------------------------------------------------------------------
def pair_index(R):
    return [(a, b) for a in range(R) for b in range(a, R)]


def chunk_sums(rows, faults=()):
    if "chunk_reversed" not in faults:
        return icp.chunk_sums(rows)
    rows = np.asarray(rows, dtype=np.float64)
    M, c = rows.shape
    n = (M + icp.CHUNK - 1) // icp.CHUNK
    pad = np.zeros((n * icp.CHUNK, c))
    pad[:M] = rows
    a = pad.reshape(n, icp.CHUNK // 256, 256, c)
    p = np.zeros((n, 256, c))
    for k in reversed(range(icp.CHUNK // 256)):
        p = p + a[:, k]
    w = 128
    while w >= 1:
        p[:, :w] = p[:, :w] + p[:, w:2 * w]
        w //= 2
    return p[:, 0]


def two_level(rows, faults=()):
    rows = np.asarray(rows, dtype=np.float64)
    if rows.shape[0] == 0:
        return np.zeros(rows.shape[1])
    if "flat_sum" in faults:
        with np.errstate(all="ignore"):
            return np.cumsum(rows, 0)[-1]
    rows = chunk_sums(rows, faults)
    while rows.shape[0] > 1:
        rows = chunk_sums(rows, faults)
    return rows[0]


def gram_terms(P, weight=None, group=1, faults=()):
    """[N, R (R + 1) / 2]: term_j = w[j / group] * (P[a][j] * P[b][j]) for the pairs a <= b row by row; exact zeros where `w > 0` is false."""
    P = np.asarray(P, dtype=np.float64)
    R, N = P.shape
    with np.errstate(all="ignore"):
        if weight is None:
            return np.stack([P[a] * P[b] for a, b in pair_index(R)], -1)
        w = np.asarray(weight, dtype=np.float64).reshape(-1)
        j = np.arange(N)
        w = w[np.minimum(j, len(w) - 1)] if "group_ignored" in faults else w[j // group]
        if "weight_first" in faults:
            out = np.stack([(w * P[a]) * P[b] for a, b in pair_index(R)], -1)
        else:
            out = np.stack([w * (P[a] * P[b]) for a, b in pair_index(R)], -1)
    return out if "keep_rejected" in faults else np.where((w > 0)[:, None], out, 0.0)


def gram(P, weight=None, group=1, faults=()):
    """The R (R + 1) / 2 sums of gram_terms, each in mofa_icp_reduce's order."""
    with np.errstate(all="ignore"):
        return two_level(gram_terms(P, weight, group, faults), faults)


def gram_matrix(sums, R):
    G = np.zeros((R, R))
    for k, (a, b) in enumerate(pair_index(R)):
        G[a, b] = G[b, a] = sums[k]
    return G


def centre(meshes):
    """(mean [n], X [M, n]): s = 0.0; s += meshes[m] (m ascending); mean = s / M; X[m] = meshes[m] - mean."""
    x = widen(meshes).reshape(len(meshes), -1)
    s = np.zeros(x.shape[1])
    for m in range(len(x)):
        s = s + x[m]
    mean = s / np.float64(len(x))
    return mean, x - mean


def combine(base, coef, rows):
    """out[b] = base + acc, acc = 0.0; acc += coef[b][r] * rows[r] (r ascending); base None: acc."""
    coef, rows = np.asarray(coef, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    out = np.zeros((coef.shape[0], rows.shape[1]))
    with np.errstate(all="ignore"):
        for b in range(coef.shape[0]):
            acc = np.zeros(rows.shape[1])
            for r in range(coef.shape[1]):
                acc = acc + coef[b, r] * rows[r]
            out[b] = acc if base is None else np.asarray(base, dtype=np.float64) + acc
    return out


def plane_rows(moved, closest, face, verts, faces, s, R, modes, faults=()):
    """P [K + 1, V]: the modes along the closest face's normal turned into the model's frame, and the residual along the normal; NaN
    columns where the face or one of its vertices lies outside the mesh."""
    v, f = widen(verts).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face = np.asarray(face, dtype=np.int64)
    y, c = widen(moved).reshape(-1, 3), widen(closest).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    modes = np.asarray(modes, dtype=np.float64).reshape(-1, len(y), 3)
    ok = (face >= 0) & (face < len(f))
    t = f[np.where(ok, face, 0)]
    ok = ok & ((t >= 0) & (t < len(v))).all(1)
    t = np.where(ok[:, None], t, 0)
    with np.errstate(all="ignore"):
        a, ab, ac = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        cr = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], -1)
        n = cr / np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])[:, None]
        if "normal_not_rotated" in faults:
            q = [np.float64(s) * n[:, k] for k in range(3)]
        else:
            q = [np.float64(s) * ((R[0, k] * n[:, 0] + R[1, k] * n[:, 1]) + R[2, k] * n[:, 2]) for k in range(3)]
        d = y - c
        rows = [(q[0] * m[:, 0] + q[1] * m[:, 1]) + q[2] * m[:, 2] for m in modes]
        rows.append((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2])
    return np.where(ok[None, :], np.stack(rows), np.nan)


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def jacobi(G, faults=()):
    """(eigenvalues [n] descending, eigenvectors [n, n] in columns, sweeps) of the symmetric G by cyclic Jacobi: sweeps over (p, q), p < q,
    row by row; a pair with A_pq == 0 is skipped, and one with |A_pp| + 100 |A_pq| == |A_pp| and the same for q, or with norm + |A_pq| == norm
    (norm: the largest |G_ii|), is set to 0 and skipped;
    otherwise theta = (A_qq - A_pp) / (2 A_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c and
    columns / rows p, q become c p - s q, s p + c q; A_pp -= t A_pq, A_qq += t A_pq.  It stops after a sweep that rotated nothing."""
    A = np.array(G, dtype=np.float64)
    n = len(A)
    W = np.eye(n)
    norm = float(np.abs(np.diag(A)).max()) if n else 0.0
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            rotated = 0
            for p in range(n - 1):
                for q in range(p + 1, n):
                    x = float(A[p, q])
                    if x == 0.0:
                        continue
                    g = 100.0 * abs(x)
                    if (abs(A[p, p]) + g == abs(A[p, p]) and abs(A[q, q]) + g == abs(A[q, q])) or norm + abs(x) == norm:
                        A[p, q] = A[q, p] = 0.0
                        continue
                    theta = (float(A[q, q]) - float(A[p, p])) / (2.0 * x)
                    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    s = t * c
                    cp, cq = A[:, p].copy(), A[:, q].copy()
                    npp, nqq = cp[p] - t * x, cq[q] + t * x
                    new_p, new_q = c * cp - s * cq, s * cp + c * cq
                    A[:, p], A[:, q] = new_p, new_q
                    A[p, :], A[q, :] = new_p, new_q
                    A[p, p], A[q, q] = npp, nqq
                    A[p, q] = A[q, p] = 0.0
                    wp, wq = W[:, p].copy(), W[:, q].copy()
                    W[:, p], W[:, q] = c * wp - s * wq, s * wp + c * wq
                    rotated += 1
            sweeps += 1
            if rotated == 0:
                break
    lam = np.diag(A).copy()
    order = list(range(n)) if "unsorted" in faults else sorted(range(n), key=lambda i: (-lam[i], i))
    lam, W = lam[order], W[:, order]
    if "no_sign_rule" not in faults:
        for k in range(n):
            if W[int(np.argmax(np.abs(W[:, k]))), k] < 0:
                W[:, k] = -W[:, k]
    return lam, W, sweeps


def cholesky_solve(A, rhs, lam=0.0):
    """x of (A + lam I) x = rhs by the written Cholesky (icp_reference.solve's loops); None when a pivot is not positive and finite or x is
    not finite.  A pivot counts as positive when it is above PIVOT_FLOOR times its diagonal entry."""
    A, rhs = np.array(A, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    n = len(rhs)
    for i in range(n):
        A[i, i] = A[i, i] + lam
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > PIVOT_FLOOR * A[j, j] and np.isfinite(s)):
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
    return x if np.isfinite(x).all() else None


def inverse_transform(s, R, t):
    """(1 / s, R^T, -(1 / s) R^T t), the last with the sum of a row left to right."""
    R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64)
    si = 1.0 / s
    return si, R.T.copy(), np.array([-(si * ((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2])) for r in range(3)])


# ---- the public calls -------------------------------------------------------------------------------------------------------------------
def shape_model(meshes, components=None, rank_tol=1e-10, align=None, align_iterations=2, faults=()):
    meshes = np.asarray(meshes, dtype=np.float32)
    M, V = meshes.shape[0], meshes.shape[1]
    transforms = None
    if align is not None:
        src, fits = meshes, [None] * M
        for _ in range(align_iterations):
            mean32 = centre(meshes)[0].reshape(V, 3).astype(np.float32)
            fits = [icp.fit_transform(src[m], mean32, model=align, metric="point", init=fits[m]) for m in range(M)]
            meshes = np.stack([f["moved"] for f in fits])
        transforms = np.stack([f["matrix"] for f in fits])
    mean, X = centre(meshes)
    G = gram_matrix(gram(X, faults=faults), M)
    lam, U, sweeps = jacobi(G, faults)
    top = float(lam.max())
    K = int(components) if components is not None else int((lam > rank_tol * top).sum())
    K = min(K, M - 1)
    pos = 0
    while pos < K and lam[pos] > 0:
        pos += 1
    K = pos
    denom = float(M if "m_not_m1" in faults else M - 1)
    sigma = np.array([math.sqrt(lam[k] / denom) for k in range(K)])
    root = np.array([math.sqrt(lam[k]) for k in range(K)])
    modes = (sigma / root)[:, None] * combine(None, U[:, :K].T.copy(), X) if K else np.zeros((0, 3 * V))
    total = 0.0
    for v in lam:
        total = total + float(v)
    out = {"mean": mean.reshape(V, 3), "modes": modes.reshape(K, V, 3), "sigma": sigma, "eigenvalues": lam, "coeffs": U[:, :K] * (root / sigma)[None, :],
           "explained": lam[:K] / total if K else np.zeros(0), "n_meshes": M, "status": "ok" if sweeps < JACOBI_SWEEPS else "sweeps"}
    if transforms is not None:
        out["transforms"] = transforms
    return out


def shape_synthesize(model, coeffs, dtype=np.float64):
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(len(coeffs), -1)
    K, V = coeffs.shape[1], model["mean"].shape[0]
    if K == 0:
        out = np.repeat(model["mean"].reshape(1, -1), len(coeffs), 0)
    else:
        out = combine(model["mean"].reshape(-1), coeffs, model["modes"][:K].reshape(K, -1))
    return out.reshape(len(coeffs), V, 3).astype(dtype)


def _normal_step(G, K, c, lam, faults=()):
    A = gram_matrix(G, K + 1)
    g = A[:K, K].copy()
    rhs = -g if ("no_lambda_c" in faults or lam == 0.0) else -(g + lam * np.asarray(c, dtype=np.float64))
    return cholesky_solve(A[:K, :K], rhs, lam), float(A[K, K])


def shape_project(model, verts, weight=None, regularize=0.0, components=None, faults=()):
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(verts)
    K = model["modes"].shape[0] if components is None else min(int(components), model["modes"].shape[0])
    w = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    w = np.where(np.isfinite(verts).all(1), w, 0.0)
    c = np.zeros(K)
    used = int((w > 0).sum())
    if used == 0:
        return {"coeffs": c, "verts": shape_synthesize(model, c[None])[0], "rms": float("nan"), "status": "empty"}
    with np.errstate(all="ignore"):
        P = np.concatenate([model["modes"][:K].reshape(K, -1), (model["mean"] - widen(verts)).reshape(1, -1)])
    wsum = two_level(w[:, None], faults)[0]
    x, _ = _normal_step(gram(P, w, 3, faults), K, c, float(regularize), faults)
    status = "ok"
    if x is None:
        x, status = c, "singular"
    recon = shape_synthesize(model, x[None])[0]
    with np.errstate(all="ignore"):
        e = gram((recon - widen(verts)).reshape(1, -1), w, 3, faults)[0]
        rms = float(np.sqrt(e / wsum))
    return {"coeffs": x, "verts": recon, "rms": rms, "status": status}


def _correspond(model, c, state, tverts, tfaces, fb, vb, weight, max_distance, reject_border, faults):
    y = shape_synthesize(model, np.asarray(c)[None])[0]
    moved = icp.apply(y.astype(np.float32), state[0], icp.q_rotation(state[1]), state[2])
    res = dist.brute_force(moved, tverts, tfaces, np.inf if max_distance is None else float(max_distance))
    finite = np.isfinite(moved).all(1) & (np.isfinite(res["d2"]) | (res["face"] < 0))
    has = finite & (res["face"] >= 0)
    on_border = has & (icp.reject(res["face"], res["bary"], tfaces, fb, vb) != 0) if reject_border else np.zeros(len(moved), dtype=bool)
    keep = has & (weight > 0) if "kept_border" in faults else has & ~on_border & (weight > 0)
    entry = {"used": int(keep.sum()), "rejected": {"non_finite": int((~finite).sum()),
                                                   "beyond" if max_distance is not None else "no_face": int((finite & ~has).sum()),
                                                   "border": int(on_border.sum())}}
    return y, moved, res, keep, entry


def shape_fit(model, target_verts, target_faces, metric="plane", pose=None, iterations=20, regularize=0.0, init=None, init_coeffs=None,
              weight=None, max_distance=None, reject_border=True, tol=0.0, components=None, faults=()):
    tverts = np.asarray(target_verts, dtype=np.float32).reshape(-1, 3)
    tfaces = np.asarray(target_faces, dtype=np.int32).reshape(-1, 3)
    V = model["mean"].shape[0]
    K = model["modes"].shape[0] if components is None else min(int(components), model["modes"].shape[0])
    weight = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    c = np.zeros(K) if init_coeffs is None else np.asarray(init_coeffs, dtype=np.float64)[:K].copy()
    state = icp.init_state(init)
    lam = float(regularize)
    modes = model["modes"][:K]

    def finish(history, done, status):
        y = shape_synthesize(model, c[None])[0]
        out = icp.result(state, icp.apply(y.astype(np.float32), state[0], icp.q_rotation(state[1]), state[2]), history, done, status)
        out["verts"] = out.pop("moved")
        out["coeffs"], out["model_verts"] = c, y
        return out

    if V == 0:
        return finish([], 0, "empty")
    if len(tverts) == 0 or len(tfaces) == 0:
        return finish([], 0, "no_correspondences")
    mu, extent = icp.box_of(tverts)
    fb, vb = icp.border_flags(tfaces, len(tverts))
    history, status, done = [], "iterations", 0
    for _ in range(iterations):
        entry = {"pose": None, "shape": None}
        history.append(entry)
        pose_step = 0.0
        if pose is not None:
            y, moved, res, keep, e = _correspond(model, c, state, tverts, tfaces, fb, vb, weight, max_distance, reject_border, faults)
            entry["pose"] = e
            w = np.where(keep, weight, 0.0)
            sums = icp.two_level(icp.terms(moved, res["closest"], w, mu, metric, face=res["face"], verts=tverts, faces=tfaces))
            new, stop = icp._update(state, sums, icp.two_level(w[:, None])[0], pose, mu, extent, e, ())
            if stop:
                status = stop
                break
            state, pose_step = new, e["step"]
        y, moved, res, keep, e = _correspond(model, c, state, tverts, tfaces, fb, vb, weight, max_distance, reject_border, faults)
        entry["shape"] = e
        e["rms"], e["step"] = float("nan"), float("nan")
        s, R, t = state[0], icp.q_rotation(state[1]), state[2]
        with np.errstate(all="ignore"):
            if metric == "plane":
                P = plane_rows(moved, res["closest"], res["face"], tverts, tfaces, s, R, modes, faults)
                keep = keep & np.isfinite(P[K])
                group = 1
            else:
                si, Ri, ti = inverse_transform(s, R, t)
                back = icp.apply(res["closest"], si, Ri, ti)
                P = np.concatenate([modes.reshape(K, -1), (y - widen(back)).reshape(1, -1)])
                keep = keep & np.isfinite(P[K].reshape(-1, 3)).all(1)
                group = 3
        e["used"] = int(keep.sum())
        w = weight if "keep_rejected" in faults else np.where(keep, weight, 0.0)
        wsum = two_level(w[:, None])[0]
        G = gram(P, w, group, faults)
        with np.errstate(all="ignore"):
            e["rms"] = float(np.sqrt(G[-1] / wsum)) if wsum > 0 else float("nan")
        if e["used"] == 0:
            status = "no_correspondences"
            break
        dc, _ = _normal_step(G, K, c, lam, faults)
        if dc is None:
            status = "singular"
            break
        c = c + dc
        e["step"] = float(np.abs(dc).max()) if K else 0.0
        done += 1
        if pose_step <= tol and e["step"] <= tol:
            status = "converged"
            break
    return finish(history, done, status)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def _entry_differs(g, w):
    if (g is None) != (w is None):
        return True
    if g is None:
        return False
    return g["used"] != w["used"] or g["rejected"] != w["rejected"] or not icp._bits(g["rms"], w["rms"]) or not icp._bits(g["step"], w["step"])


def mismatches(got, want):
    """The parts of a result of shape_model / shape_project / shape_fit (tensors on the host) that differ from ``want`` in any bit."""
    bad = []
    for k, w in want.items():
        if k == "history":
            if len(got[k]) != len(w):
                bad.append("history length")
                continue
            bad += [f"history[{i}].{ph}" for i, (a, b) in enumerate(zip(got[k], w)) for ph in ("pose", "shape") if _entry_differs(a[ph], b[ph])]
        elif isinstance(w, (str, int)) and not isinstance(w, bool):
            if got[k] != w:
                bad.append(k)
        elif isinstance(w, float):
            if not icp._bits(got[k], w):
                bad.append(k)
        elif not dist._same(np.asarray(got[k]), np.asarray(w)):
            bad.append(k)
    return bad


# ---- the scene --------------------------------------------------------------------------------------------------------------------------
N_GRID = 13
MEMBERS_CENTRE, MEMBERS_SPREAD, UNSEEN = np.array([0.6, 0.25, -0.2]), 0.3, np.array([0.45, 0.4, -0.05])
_cache = {}


def field_faces(n):
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    v00 = (i * n + j).reshape(-1)
    v10, v01, v11 = v00 + n, v00 + 1, v00 + n + 1
    return np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32)


def member(a, n=N_GRID):
    """The height field z = a1 g1 + a2 g2 + a3 g3 + 0.1 x y + 0.15 x on an n x n lattice of [-1, 1]^2 (g: icp_reference.patch's Gaussians)."""
    g = np.linspace(-1.0, 1.0, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = (a[0] * np.exp(-((x - 0.1) ** 2 + (y + 0.2) ** 2) / 0.15) + a[1] * np.exp(-((x + 0.45) ** 2 + (y - 0.35) ** 2) / 0.05)
         + a[2] * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.08) + 0.1 * x * y + 0.15 * x)
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def family():
    """[8, 169, 3] float32: eight seeded members within +-0.3 of (0.6, 0.25, -0.2)."""
    if "family" not in _cache:
        rng = np.random.default_rng(7)
        _cache["family"] = np.stack([member(MEMBERS_CENTRE + MEMBERS_SPREAD * rng.uniform(-1, 1, 3)) for _ in range(8)])
    return _cache["family"]


def model():
    if "model" not in _cache:
        _cache["model"] = shape_model(family())
    return _cache["model"]


def subdivide(verts, faces):
    """One 1-to-4 midpoint subdivision (midpoints in fp64, rounded to float32: exact for the lattice coordinates used here)."""
    v = [tuple(r) for r in widen(verts)]
    ids, out = {}, []

    def mid(a, b):
        key = (min(a, b), max(a, b))
        if key not in ids:
            ids[key] = len(v)
            v.append(tuple((np.array(v[a]) + np.array(v[b])) * 0.5))
        return ids[key]

    for a, b, c in np.asarray(faces, dtype=np.int64):
        ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.array(v, dtype=np.float32), np.array(out, dtype=np.int32)


def target(cropped=False):
    """The unseen member's own mesh after one subdivision: 625 vertices, 1,152 faces; ``cropped``: its faces with centroid x < 0.4."""
    if "target" not in _cache:
        _cache["target"] = subdivide(member(UNSEEN), field_faces(N_GRID))
    verts, faces = _cache["target"]
    if cropped:
        faces = faces[widen(verts)[faces.astype(np.int64)].mean(1)[:, 0] < 0.4].copy()
    return verts, faces


def rms_error(verts, truth):
    d = np.asarray(verts, dtype=np.float64) - widen(truth)
    return float(np.sqrt((d * d).sum(1).mean()))
