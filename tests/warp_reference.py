"""NumPy restatement of the non-rigid mesh registration (include/mofanerf_hip.h, mofa_warp_*; mofanerf_amd.mesh.warp_to /
warp): the apply, the per-vertex system for both metrics, the product with D + alpha L (x) I3 in the adjacency's order, the inner product
through icp_reference.two_level, the Jacobi-preconditioned conjugate gradients with their sticky freeze, and the two host functions, with the
closest points taken from dist_reference.brute_force, the border rule from icp_reference and the adjacency from smooth_reference.  Test code,
not product.  ``mismatches`` is THE comparison of a result; tests/test_warp_reference_cpu.py shows that every injected fault (``faults``: a
set of the names in FAULTS) changes the result of a catalogue case."""
import numpy as np

import dist_reference as dist
import icp_reference as icp
import smooth_reference as smooth

FAULTS = ("reversed_order", "no_degree", "unsymmetric", "no_point_weight", "no_warm_start", "no_preconditioner", "stale_rho",
          "freeze_not_sticky", "keep_border", "handles_no_rhs")
STOPS = {0: "iterations", 1: "tolerance", 2: "breakdown"}
widen = dist.widen


# ---- the device side --------------------------------------------------------------------------------------------------------------------
def apply(verts, d):
    """y = (float)((double)v + d)"""
    with np.errstate(all="ignore"):
        return (widen(verts).reshape(-1, 3) + np.asarray(d, dtype=np.float64).reshape(-1, 3)).astype(np.float32)


def adjacency(faces, V, faults=()):
    return smooth.adjacency(faces, V, "reversed_order" if "reversed_order" in faults else None)


def degree(adj):
    return np.diff(adj["offsets"]).astype(np.float64)


def system(verts, moved, target, weight, adj, metric, alpha, point_weight=1e-2, normals=None, face=None, tverts=None, tfaces=None,
           hweight=None, hpos=None, faults=()):
    """(D [V,6]: xx xy xz yy yz zz, b [V,3], minv [V,3], e [V]) of mofa_warp_system."""
    v, y, c = widen(verts).reshape(-1, 3), widen(moved).reshape(-1, 3), widen(target).reshape(-1, 3)
    w = np.asarray(weight, dtype=np.float64).reshape(-1)
    V = len(v)
    live = w > 0
    pw = 0.0 if "no_point_weight" in faults else float(point_weight)
    D, b = np.zeros((V, 6)), np.zeros((V, 3))
    with np.errstate(all="ignore"):
        u, r = c - v, y - c
        rr = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        if metric == "plane":
            if face is not None:
                n, ok = icp.face_normals(tverts, tfaces, face)
                live = live & ok
            else:
                n = widen(normals).reshape(-1, 3)
            for col, (k, l) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                D[:, col] = w * (n[:, k] * n[:, l] + pw) if k == l else w * (n[:, k] * n[:, l])
            nu = (n[:, 0] * u[:, 0] + n[:, 1] * u[:, 1]) + n[:, 2] * u[:, 2]
            nr = (n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]
            for k in range(3):
                b[:, k] = w * (n[:, k] * nu + pw * u[:, k])
            e = w * (nr * nr + pw * rr)
        elif metric == "point":
            D[:, 0] = D[:, 3] = D[:, 5] = w
            for k in range(3):
                b[:, k] = w * u[:, k]
            e = w * rr
        else:
            raise ValueError(metric)
    D, b, e = np.where(live[:, None], D, 0.0), np.where(live[:, None], b, 0.0), np.where(live, e, 0.0)
    if hweight is not None:
        h = np.asarray(hweight, dtype=np.float64).reshape(-1)
        on = h > 0
        hp = widen(hpos).reshape(-1, 3)
        with np.errstate(all="ignore"):
            for col in (0, 3, 5):
                D[:, col] = np.where(on, D[:, col] + h, D[:, col])
            if "handles_no_rhs" not in faults:
                for k in range(3):
                    b[:, k] = np.where(on, b[:, k] + h * (hp[:, k] - v[:, k]), b[:, k])
    ad = float(alpha) * (0.0 * degree(adj) if "no_degree" in faults else degree(adj))
    with np.errstate(all="ignore"):
        m = np.stack([D[:, 0] + ad, D[:, 3] + ad, D[:, 5] + ad], -1)
        minv = np.where(m > 0, 1.0 / np.where(m > 0, m, 1.0), 0.0)
    return D, b, minv, e


def neighbour_sums(p, adj):
    """s_i = 0.0 + p_j over the list of i in its order, [V,3]."""
    off, nbr = adj["offsets"], adj["neighbours"].astype(np.int64)
    deg = np.diff(off)
    s = np.zeros_like(p)
    with np.errstate(all="ignore"):
        for k in range(int(deg.max()) if len(deg) else 0):
            has = deg > k
            j = nbr[np.where(has, off[:-1] + k, 0)] if len(nbr) else np.zeros(len(deg), dtype=np.int64)
            s = np.where(has[:, None], s + p[j], s)
    return s


def matvec(D, p, adj, alpha, faults=()):
    """q = (D + alpha L (x) I3) p in mofa_warp_matvec's order."""
    deg = 0.0 * degree(adj) if "no_degree" in faults else degree(adj)
    s = neighbour_sums(p, adj)
    yx = D[:, 2] if "unsymmetric" in faults else D[:, 1]
    with np.errstate(all="ignore"):
        Dp = [(D[:, 0] * p[:, 0] + D[:, 1] * p[:, 1]) + D[:, 2] * p[:, 2], (yx * p[:, 0] + D[:, 3] * p[:, 1]) + D[:, 4] * p[:, 2],
              (D[:, 2] * p[:, 0] + D[:, 4] * p[:, 1]) + D[:, 5] * p[:, 2]]
        return np.stack([Dp[k] + float(alpha) * (deg * p[:, k] - s[:, k]) for k in range(3)], -1)


def dot_terms(a, b):
    with np.errstate(all="ignore"):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def dot(a, b, faults=()):
    """The inner product of two [V,3] vectors: the per-vertex terms summed as mofa_icp_reduce sums one column."""
    return float(icp.two_level(dot_terms(a, b)[:, None], faults)[0])


def cg(D, b, minv, adj, alpha, x0, cg_iterations, cg_tol, faults=()):
    """(x, record) of mofa_warp_solve: record = {"rho": [K + 1], "steps", "stop", "a", "p", "r"}."""
    K, tol2 = int(cg_iterations), float(cg_tol) * float(cg_tol)
    if "no_preconditioner" in faults:
        minv = np.ones_like(minv)
    x = np.array(x0, dtype=np.float64).reshape(-1, 3).copy()
    with np.errstate(all="ignore"):
        r = b - matvec(D, x, adj, alpha, faults)
        z = minv * r
        p = z.copy()
        rho_s = dot(r, z)
        rho0, rho_prev = rho_s, rho_s
        rho, frozen, cause, steps, a = [], False, 0, 0, 0.0
        for s in range(K):
            rho.append(rho_s)
            if "freeze_not_sticky" in faults:
                frozen = False
            if not frozen:
                q = matvec(D, p, adj, alpha, faults)
                pq = dot(p, q)
                if rho_s <= tol2 * rho0:
                    frozen, cause = True, 1
                elif not pq > 0:
                    frozen, cause = True, 2
                else:
                    a, steps = (rho_prev if "stale_rho" in faults else rho_s) / pq, s + 1
            if frozen:
                a = 0.0
                if "freeze_not_sticky" not in faults:
                    continue
            x = x + a * p
            r = r - a * q
            z = minv * r
            rho_new = dot(r, z)
            p = z + (rho_new / rho_s) * p
            rho_prev, rho_s = rho_s, rho_new
        rho.append(rho_s)
    return x, {"rho": np.array(rho), "steps": steps, "stop": STOPS[cause], "a": a, "p": p, "r": r}


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _solve_record(rec):
    return {"rho": rec["rho"], "steps": rec["steps"], "stop": rec["stop"]}


def warp_to(verts, faces, targets, weight=None, normals=None, metric="point", stiffness=1.0, point_weight=1e-2, init=None, cg_iterations=200,
            cg_tol=1e-8, faults=()):
    verts, faces = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V = len(verts)
    d = np.zeros((V, 3)) if init is None else np.array(init, dtype=np.float64).reshape(V, 3)
    if V == 0:
        return verts.copy(), d, {"rho": np.zeros(0), "steps": 0, "stop": "iterations"}
    weight = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    adj = adjacency(faces, V, faults)
    D, b, minv, _ = system(verts, apply(verts, d), targets, weight, adj, metric, stiffness, point_weight, normals=normals, faults=faults)
    x, rec = cg(D, b, minv, adj, stiffness, np.zeros((V, 3)) if "no_warm_start" in faults else d, cg_iterations, cg_tol, faults)
    return apply(verts, x), x, _solve_record(rec)


def handle_arrays(handles, V):
    """(hweight [V] float64, hpos [V,3] float32) of ``handles = (index, position, weight)``, or (None, None)."""
    if handles is None:
        return None, None
    index, pos, hw = handles
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    hweight, hpos = np.zeros(V), np.zeros((V, 3), dtype=np.float32)
    hweight[index] = np.broadcast_to(np.asarray(hw, dtype=np.float64), index.shape)
    hpos[index] = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    return hweight, hpos


def step_size(x, d):
    with np.errstate(all="ignore"):
        t = x - d
        return float(np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]).max())


def warp(verts, faces, target_verts, target_faces, metric="plane", stiffness=(10.0, 1.0, 0.1), iterations=5, point_weight=1e-2, weight=None,
         handles=None, max_distance=None, reject_border=True, init=None, tol=0.0, cg_iterations=200, cg_tol=1e-8, faults=()):
    verts, faces = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    tv, tf = np.asarray(target_verts, dtype=np.float32).reshape(-1, 3), np.asarray(target_faces, dtype=np.int32).reshape(-1, 3)
    V = len(verts)
    d = np.zeros((V, 3)) if init is None else np.array(init, dtype=np.float64).reshape(V, 3)
    out = lambda history, done, status: {"verts": apply(verts, d), "displacement": d, "history": history, "iterations": done, "status": status}
    if V == 0:
        return out([], 0, "empty")
    if len(tv) == 0 or len(tf) == 0:
        return out([], 0, "no_correspondences")
    weight = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    hweight, hpos = handle_arrays(handles, V)
    adj = adjacency(faces, V, faults)
    _, extent = icp.box_of(tv)
    fb, vb = icp.border_flags(tf, len(tv))
    history, status, done = [], "iterations", 0
    for alpha in np.atleast_1d(np.asarray(stiffness, dtype=np.float64)):
        status = "iterations"
        for _ in range(iterations):
            y = apply(verts, d)
            res = dist.brute_force(y, tv, tf, np.inf if max_distance is None else float(max_distance))
            finite = np.isfinite(y).all(1) & (np.isfinite(res["d2"]) | (res["face"] < 0))
            has = finite & (res["face"] >= 0)
            on_border = has & (icp.reject(res["face"], res["bary"], tf, fb, vb) != 0) if reject_border else np.zeros(V, dtype=bool)
            keep = (has if "keep_border" in faults else has & ~on_border) & (weight > 0)
            w = np.where(keep, weight, 0.0)
            entry = {"stiffness": float(alpha), "rms": float("nan"), "used": int(keep.sum()),
                     "rejected": {"non_finite": int((~finite).sum()), "beyond" if max_distance is not None else "no_face": int((finite & ~has).sum()),
                                  "border": int(on_border.sum())}, "cg_steps": 0, "rho": float("nan"), "stop": None, "step": float("nan")}
            history.append(entry)
            D, b, minv, e = system(verts, y, res["closest"], w, adj, metric, alpha, point_weight, face=res["face"], tverts=tv, tfaces=tf,
                                   hweight=hweight, hpos=hpos, faults=faults)
            sum_e, sum_w = icp.two_level(e[:, None])[0], icp.two_level(w[:, None])[0]
            with np.errstate(all="ignore"):
                entry["rms"] = float(np.sqrt(sum_e / sum_w)) if sum_w > 0 else float("nan")
            if entry["used"] == 0:
                return out(history, done, "no_correspondences")
            x, rec = cg(D, b, minv, adj, alpha, np.zeros((V, 3)) if "no_warm_start" in faults else d, cg_iterations, cg_tol, faults)
            entry["cg_steps"], entry["rho"], entry["stop"] = rec["steps"], float(rec["rho"][-1]), rec["stop"]
            if rec["stop"] == "breakdown" and rec["steps"] == 0 and rec["rho"][0] > 0:
                return out(history, done, "singular")
            entry["step"] = step_size(x, d)
            d, done = x, done + 1
            if entry["step"] <= tol * extent:
                status = "converged"
                break
    return out(history, done, status)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
_bits = icp._bits


def solve_mismatches(got, want):
    bad = [] if _bits(got["rho"], want["rho"]) else ["rho"]
    return bad + [k for k in ("steps", "stop") if got[k] != want[k]]


def mismatches(got, want):
    """The parts of a warp result (``verts`` / ``displacement`` on the host) that differ from ``want`` in any bit."""
    bad = []
    if np.asarray(got["verts"]).dtype != np.float32 or not dist._same(np.asarray(got["verts"]), np.asarray(want["verts"])):
        bad.append("verts")
    if not dist._same(np.asarray(got["displacement"]), np.asarray(want["displacement"])):
        bad.append("displacement")
    bad += [k for k in ("status", "iterations") if got[k] != want[k]]
    if len(got["history"]) != len(want["history"]):
        return bad + ["history length"]
    for i, (g, w) in enumerate(zip(got["history"], want["history"])):
        same = all(g[k] == w[k] for k in ("used", "rejected", "cg_steps", "stop")) and all(_bits(g[k], w[k]) for k in ("stiffness", "rms", "rho", "step"))
        if not same:
            bad.append(f"history[{i}]")
    return bad


# ---- the scene catalogue ----------------------------------------------------------------------------------------------------------------
_cache = {}


def template(n=13):
    """The template of the patch scenes: an n x n grid on [-1, 1]^2 that carries only the patch's low-frequency terms
    (z = 0.1 x y + 0.15 x), two faces per cell in the patch's own pattern: 169 vertices, 288 faces at n = 13."""
    if ("template", n) not in _cache:
        g = np.linspace(-1.0, 1.0, n)
        x, y = np.meshgrid(g, g, indexing="ij")
        verts = np.stack([x, y, 0.1 * x * y + 0.15 * x], -1).reshape(-1, 3).astype(np.float32)
        i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
        v00 = (i * n + j).reshape(-1)
        v10, v01, v11 = v00 + n, v00 + 1, v00 + n + 1
        _cache["template", n] = (verts, np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32))
    return _cache["template", n]


def scene(name):
    """(template verts, template faces, target verts, target faces) of "patch" or "crop"."""
    return template() + (icp.patch() if name == "patch" else icp.crop())


def isolated():
    """The tetrahedron plus a vertex (4) that no face references."""
    verts, faces = smooth.tetrahedron()
    return np.concatenate([verts, np.array([[0.5, 0.25, 2.0]], dtype=np.float32)]), faces


SOLVER_MESHES = (("strip1", lambda: (smooth.strip(3)[0][:1].copy(), np.zeros((0, 3), dtype=np.int32))), ("strip2", lambda: _strip2()),
                 ("strip5", lambda: smooth.strip(5)), ("strip257", lambda: smooth.strip(257)), ("tetrahedron", smooth.tetrahedron),
                 ("odd_mesh", smooth.odd_mesh), ("isolated", isolated))


def _strip2():
    verts, _ = smooth.strip(3)
    return verts[:2].copy(), np.array([[0, 0, 1]], dtype=np.int32)       # a degenerate face still makes 0 and 1 neighbours


def strip(V):
    """smooth_reference.strip for any V >= 1 (V < 3: no proper face)."""
    if V == 1:
        return SOLVER_MESHES[0][1]()
    if V == 2:
        return _strip2()
    if V <= 4096:
        return smooth.strip(V)
    k = np.arange(V)                                                      # the same strip without the Python loop over its faces
    verts = np.stack([0.5 * k, k % 2, 0.2 * np.random.default_rng(2).standard_normal(V)], -1).astype(np.float32)
    i = np.arange(V - 2)
    even = (i % 2 == 0)
    return verts, np.stack([np.where(even, i, i + 1), np.where(even, i + 1, i), i + 2], -1).astype(np.int32)


def solver_case(mesh, seed=0):
    """(verts, faces, targets float32, weight float64 > 0 except where the vertex has no neighbour in "isolated", unit normals float32) of a
    mesh (a name of SOLVER_MESHES or a (verts, faces) pair): targets = the vertices moved by a smooth field plus noise from ``seed``."""
    verts, faces = dict(SOLVER_MESHES)[mesh]() if isinstance(mesh, str) else mesh
    verts = np.asarray(verts, dtype=np.float32)
    V = len(verts)
    rng = np.random.default_rng(seed + V)
    v = widen(verts)
    field = np.stack([0.2 * np.sin(1.3 * v[:, 1] + 0.1), 0.15 * np.cos(0.7 * v[:, 0]), 0.25 * np.sin(0.9 * v[:, 0] + 0.5 * v[:, 1])], -1)
    targets = (v + field + 0.02 * rng.standard_normal((V, 3))).astype(np.float32)
    weight = 0.5 + rng.random(V)
    if mesh == "isolated":
        weight[4] = 0.0
    n = rng.standard_normal((V, 3)) + np.array([0.0, 0.0, 2.0])
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return verts, np.asarray(faces, dtype=np.int32).reshape(-1, 3), targets, weight, normals
