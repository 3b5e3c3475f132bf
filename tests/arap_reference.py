"""NumPy restatement of the as-rigid-as-possible stiffness (include/mofanerf_hip.h, mofa_warp_rotations / mofa_warp_arap_rhs; DESIGN.md 3.24;
mofanerf_amd.mesh.warp(stiffness_model="arap") / mesh.deform): the per-vertex rotation fit — Horn's 4 x 4 matrix of the neighbourhood's
covariance, its eigenvector of the largest eigenvalue by cyclic Jacobi with a fixed number of sweeps, the rotation of that quaternion —, the
rotation term of the right-hand side, and the two host loops, vectorised over the vertices with masks as warp_reference.neighbour_sums is.
The system, the conjugate gradients and the apply are warp_reference's, the closest points dist_reference.brute_force's, the border rule
and the two-level sum icp_reference's.  Test code, not product.  ``mismatches`` is THE comparison of a result;
tests/test_arap_reference_cpu.py shows that every injected fault (``faults``: a set of the names in FAULTS) changes a catalogue result."""
import numpy as np

import dist_reference as dist
import icp_reference as icp
import smooth_reference as smooth
import warp_reference as wr

FAULTS = ("transposed_covariance", "no_average", "reversed_order", "one_sweep", "smallest_eigenvalue", "rhs_not_scaled", "rest_pose_rotations",
          "moved_float32", "tie_highest_index")
SWEEPS = 7               # MOFA_WARP_JACOBI_SWEEPS
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
widen = dist.widen


# ---- the device side --------------------------------------------------------------------------------------------------------------------
def slots(adj):
    """Per position k of the lists: (has [V] bool: the list of i is longer than k, j [V]: its k-th neighbour, 0 where it has none)."""
    off, nbr = adj["offsets"], adj["neighbours"].astype(np.int64)
    deg = np.diff(off)
    for k in range(int(deg.max()) if len(deg) else 0):
        has = deg > k
        yield has, (nbr[np.where(has, off[:-1] + k, 0)] if len(nbr) else np.zeros(len(deg), dtype=np.int64))


def edge_pairs(v, d, adj, faults=()):
    """Per position of the lists: (has, j, e = v_i - v_j, e' = e + (d_i - d_j))."""
    y = widen(wr.apply(v.astype(np.float32), d)) if "moved_float32" in faults else None
    with np.errstate(all="ignore"):
        for has, j in slots(adj):
            e = v - v[j]
            yield has, j, e, ((y - y[j]) if y is not None else e + (d - d[j]))


def covariance(v, d, adj, faults=()):
    """S [V,3,3]: S_ab = 0.0 + e_a e'_b over the list in its order."""
    S = np.zeros((len(v), 3, 3))
    with np.errstate(all="ignore"):
        for has, _, e, ep in edge_pairs(v, d, adj, faults):
            term = ep[:, :, None] * e[:, None, :] if "transposed_covariance" in faults else e[:, :, None] * ep[:, None, :]
            S = np.where(has[:, None, None], S + term, S)
    return S


def horn(S):
    """N [V,4,4] (symmetric) of the header."""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[:, a, b] for a in range(3) for b in range(3))
    with np.errstate(all="ignore"):
        rows = [[(xx + yy) + zz, yz - zy, zx - xz, xy - yx], [None, (xx - yy) - zz, xy + yx, zx + xz], [None, None, (yy - xx) - zz, yz + zy],
                [None, None, None, (zz - xx) - yy]]
    N = np.zeros((len(S), 4, 4))
    for p in range(4):
        for q in range(p, 4):
            N[:, p, q] = N[:, q, p] = rows[p][q]
    return N


def jacobi(N, sweeps=SWEEPS):
    """(a [V,4,4], v [V,4,4]) after ``sweeps`` cyclic sweeps over PAIRS: the header's rotation, skipped where a_pq == 0."""
    a, v = np.array(N, dtype=np.float64), np.broadcast_to(np.eye(4), N.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = a[:, p, q].copy()
                on = apq != 0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                new = a.copy()
                new[:, p, p], new[:, q, q] = a[:, p, p] - t * apq, a[:, q, q] + t * apq
                new[:, p, q] = new[:, q, p] = 0.0
                for k in range(4):
                    if k != p and k != q:
                        new[:, k, p] = new[:, p, k] = c * a[:, k, p] - s * a[:, k, q]
                        new[:, k, q] = new[:, q, k] = s * a[:, k, p] + c * a[:, k, q]
                nv = v.copy()
                nv[:, :, p], nv[:, :, q] = c[:, None] * v[:, :, p] - s[:, None] * v[:, :, q], s[:, None] * v[:, :, p] + c[:, None] * v[:, :, q]
                a, v = np.where(on[:, None, None], new, a), np.where(on[:, None, None], nv, v)
    return a, v


def off_norm(a):
    """The relative off-diagonal norm of [V,4,4] matrices (0 for a zero matrix)."""
    off = np.sqrt(sum(2.0 * a[:, p, q] * a[:, p, q] for p, q in PAIRS))
    full = np.sqrt((a * a).sum((1, 2)))
    return np.where(full > 0, off / np.where(full > 0, full, 1.0), 0.0)


def quat_rotation(q):
    """[V,9] of unit quaternions [V,4]: mesh._quat_rotation's operations."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        return np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], -1)


def rotations(verts, d, adj, faults=(), sweeps=None):
    """(R [V,9] row-major, fit [V], n_non_finite) of mofa_warp_rotations."""
    v, d = widen(verts).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    V = len(v)
    sweeps = (1 if "one_sweep" in faults else SWEEPS) if sweeps is None else sweeps
    S = covariance(v, d, adj, faults)
    finite = np.isfinite(S).all((1, 2))
    a, vec = jacobi(horn(np.where(finite[:, None, None], S, 0.0)), sweeps)
    diag = np.einsum("vkk->vk", a)
    if "smallest_eigenvalue" in faults:
        diag = -diag
    m = np.zeros(V, dtype=np.int64)
    best = diag[:, 0].copy()
    for k in (1, 2, 3):
        better = diag[:, k] >= best if "tie_highest_index" in faults else diag[:, k] > best
        m, best = np.where(better, k, m), np.where(better, diag[:, k], best)
    q = vec[np.arange(V), :, m]
    with np.errstate(all="ignore"):
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        R = quat_rotation(q / n[:, None])
    good = finite & np.isfinite(R).all(1)
    R = np.where(good[:, None], R, IDENTITY)
    fit = np.zeros(V)
    with np.errstate(all="ignore"):
        for has, _, e, ep in edge_pairs(v, d, adj, faults):
            r = [ep[:, c] - ((R[:, 3 * c] * e[:, 0] + R[:, 3 * c + 1] * e[:, 1]) + R[:, 3 * c + 2] * e[:, 2]) for c in range(3)]
            fit = np.where(has, fit + ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]), fit)
    return R, np.where(good, fit, 0.0), int((~good).sum())


def arap_g(verts, R, adj, faults=()):
    """g [V,3]: per neighbour Rs = R_i + R_j, t_c = (Rs_c0 e_0 + Rs_c1 e_1) + Rs_c2 e_2, g_c += 0.5 t_c - e_c."""
    v = widen(verts).reshape(-1, 3)
    g = np.zeros((len(v), 3))
    with np.errstate(all="ignore"):
        for has, j in slots(adj):
            e = v - v[j]
            Rs = R + (R if "no_average" in faults else R[j])
            t = np.stack([(Rs[:, 3 * c] * e[:, 0] + Rs[:, 3 * c + 1] * e[:, 1]) + Rs[:, 3 * c + 2] * e[:, 2] for c in range(3)], -1)
            g = np.where(has[:, None], g + (0.5 * t - e), g)
    return g


def arap_rhs(verts, R, adj, alpha, b, faults=()):
    """b + alpha g of mofa_warp_arap_rhs (a new array)."""
    with np.errstate(all="ignore"):
        return b + (1.0 if "rhs_not_scaled" in faults else float(alpha)) * arap_g(verts, R, adj, faults)


def energy(fit):
    """arap_energy: half of the two-level sum of fit."""
    return 0.5 * float(icp.two_level(np.asarray(fit, dtype=np.float64)[:, None])[0])


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _adjacency(faces, V, faults):
    return smooth.adjacency(faces, V, "reversed_order" if "reversed_order" in faults else None)


def _fit(verts, d, adj, faults):
    return rotations(verts, np.zeros_like(d) if "rest_pose_rotations" in faults else d, adj, faults)


def deform(verts, faces, handles, stiffness=1.0, iterations=40, init=None, tol=0.0, cg_iterations=200, cg_tol=1e-8, faults=()):
    verts, faces = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V, alpha = len(verts), float(stiffness)
    d = np.zeros((V, 3)) if init is None else np.array(init, dtype=np.float64).reshape(V, 3)
    R = np.tile(IDENTITY, (V, 1))
    out = lambda history, done, status: {"verts": wr.apply(verts, d), "displacement": d, "rotations": R.reshape(V, 3, 3), "history": history,
                                         "iterations": done, "status": status}
    if V == 0:
        return out([], 0, "empty")
    hweight, hpos = wr.handle_arrays(handles, V)
    adj = _adjacency(faces, V, faults)
    _, extent = icp.box_of(verts)
    history, status, done = [], "iterations", 0
    for _ in range(iterations):
        Rn, fit, _ = _fit(verts, d, adj, faults)
        entry = {"arap_energy": energy(fit), "cg_steps": 0, "rho": float("nan"), "stop": None, "step": float("nan")}
        history.append(entry)
        D, b, minv, _ = wr.system(verts, verts, verts, np.zeros(V), adj, "point", alpha, hweight=hweight, hpos=hpos)
        b = arap_rhs(verts, Rn, adj, alpha, b, faults)
        x, rec = wr.cg(D, b, minv, adj, alpha, d, cg_iterations, cg_tol)
        entry["cg_steps"], entry["rho"], entry["stop"] = rec["steps"], float(rec["rho"][-1]), rec["stop"]
        if rec["stop"] == "breakdown" and rec["steps"] == 0 and rec["rho"][0] > 0:
            return out(history, done, "singular")
        entry["step"] = wr.step_size(x, d)
        d, R, done = x, Rn, done + 1
        if entry["step"] <= tol * extent:
            status = "converged"
            break
    return out(history, done, status)


def warp(verts, faces, target_verts, target_faces, metric="plane", stiffness=(10.0, 1.0, 0.1), iterations=5, point_weight=1e-2, weight=None,
         handles=None, max_distance=None, reject_border=True, init=None, tol=0.0, cg_iterations=200, cg_tol=1e-8, stiffness_model="displacement",
         faults=()):
    """warp_reference.warp with the model switch: "arap" fits the rotations to d before every solve and amends the right-hand side."""
    if stiffness_model not in ("displacement", "arap"):
        raise ValueError(stiffness_model)
    arap = stiffness_model == "arap"
    verts, faces = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    tv, tf = np.asarray(target_verts, dtype=np.float32).reshape(-1, 3), np.asarray(target_faces, dtype=np.int32).reshape(-1, 3)
    V = len(verts)
    d = np.zeros((V, 3)) if init is None else np.array(init, dtype=np.float64).reshape(V, 3)
    R = np.tile(IDENTITY, (V, 1))

    def out(history, done, status):
        res = {"verts": wr.apply(verts, d), "displacement": d, "history": history, "iterations": done, "status": status}
        if arap:
            res["rotations"] = R.reshape(V, 3, 3)
        return res

    if V == 0:
        return out([], 0, "empty")
    if len(tv) == 0 or len(tf) == 0:
        return out([], 0, "no_correspondences")
    weight = np.ones(V) if weight is None else np.asarray(weight, dtype=np.float64)
    hweight, hpos = wr.handle_arrays(handles, V)
    adj = _adjacency(faces, V, faults)
    _, extent = icp.box_of(tv)
    fb, vb = icp.border_flags(tf, len(tv))
    history, status, done = [], "iterations", 0
    for alpha in np.atleast_1d(np.asarray(stiffness, dtype=np.float64)):
        status = "iterations"
        for _ in range(iterations):
            y = wr.apply(verts, d)
            res = dist.brute_force(y, tv, tf, np.inf if max_distance is None else float(max_distance))
            finite = np.isfinite(y).all(1) & (np.isfinite(res["d2"]) | (res["face"] < 0))
            has = finite & (res["face"] >= 0)
            on_border = has & (icp.reject(res["face"], res["bary"], tf, fb, vb) != 0) if reject_border else np.zeros(V, dtype=bool)
            keep = has & ~on_border & (weight > 0)
            w = np.where(keep, weight, 0.0)
            entry = {"stiffness": float(alpha), "rms": float("nan"), "used": int(keep.sum()),
                     "rejected": {"non_finite": int((~finite).sum()), "beyond" if max_distance is not None else "no_face": int((finite & ~has).sum()),
                                  "border": int(on_border.sum())}, "cg_steps": 0, "rho": float("nan"), "stop": None, "step": float("nan")}
            history.append(entry)
            D, b, minv, e = wr.system(verts, y, res["closest"], w, adj, metric, alpha, point_weight, face=res["face"], tverts=tv, tfaces=tf,
                                      hweight=hweight, hpos=hpos)
            if arap:
                Rn, fit, _ = _fit(verts, d, adj, faults)
                b = arap_rhs(verts, Rn, adj, alpha, b, faults)
                entry["arap_energy"] = energy(fit)
            sum_e, sum_w = icp.two_level(e[:, None])[0], icp.two_level(w[:, None])[0]
            with np.errstate(all="ignore"):
                entry["rms"] = float(np.sqrt(sum_e / sum_w)) if sum_w > 0 else float("nan")
            if entry["used"] == 0:
                return out(history, done, "no_correspondences")
            x, rec = wr.cg(D, b, minv, adj, alpha, d, cg_iterations, cg_tol)
            entry["cg_steps"], entry["rho"], entry["stop"] = rec["steps"], float(rec["rho"][-1]), rec["stop"]
            if rec["stop"] == "breakdown" and rec["steps"] == 0 and rec["rho"][0] > 0:
                return out(history, done, "singular")
            entry["step"] = wr.step_size(x, d)
            d, done = x, done + 1
            if arap:
                R = Rn
            if entry["step"] <= tol * extent:
                status = "converged"
                break
    return out(history, done, status)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
_bits = icp._bits


def mismatches(got, want):
    """The parts of a result of warp(stiffness_model="arap") or deform (tensors on the host) that differ from ``want`` in any bit."""
    bad = []
    if np.asarray(got["verts"]).dtype != np.float32 or not dist._same(np.asarray(got["verts"]), np.asarray(want["verts"])):
        bad.append("verts")
    bad += [k for k in ("displacement", "rotations") if (k in got) != (k in want) or (k in got and not dist._same(np.asarray(got[k]), np.asarray(want[k])))]
    bad += [k for k in ("status", "iterations") if got[k] != want[k]]
    if len(got["history"]) != len(want["history"]):
        return bad + ["history length"]
    for i, (g, w) in enumerate(zip(got["history"], want["history"])):
        same = set(g) == set(w) and all(g[k] == w[k] for k in ("used", "rejected", "cg_steps", "stop") if k in w)
        same = same and all(_bits(g[k], w[k]) for k in ("stiffness", "rms", "rho", "step", "arap_energy") if k in w)
        if not same:
            bad.append(f"history[{i}]")
    return bad


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
def rotation_about(axis, angle_deg):
    """Rodrigues' matrix (test data, not the product's path)."""
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def flat(n=5):
    """An n x n grid in the plane z = 0.25 (every neighbourhood exactly rank 2), the template's face pattern."""
    verts, faces = wr.template(n)
    verts = verts.copy()
    verts[:, 2] = 0.25
    return verts, faces


def grid_patch(n=9):
    """The deform scene's patch: an n x n grid on [0, 1]^2 with z = 0.05 sin 3x cos 2y."""
    g = np.linspace(0.0, 1.0, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([x, y, 0.05 * np.sin(3 * x) * np.cos(2 * y)], -1).reshape(-1, 3).astype(np.float32)
    return verts, wr.template(n)[1]


def border_of(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.flatnonzero(((i == 0) | (i == n - 1) | (j == 0) | (j == n - 1)).reshape(-1))


AXES = ((1.0, 2.0, 2.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), tuple(icp.AXIS))
ANGLES = (1.0, 90.0, 179.0, 180.0)
MESHES = dict(wr.SOLVER_MESHES, flat=flat, template=wr.template)
_cases = {}


def rigid_displacement(verts, R, t):
    v = widen(verts)
    return v @ R.T + np.asarray(t) - v


def catalogue():
    """{name: (verts float32, faces int32, d float64, truth)}; truth: the rotation [3,3] of an exact rigid motion, else None."""
    if _cases:
        return _cases
    for name, make in MESHES.items():
        verts, faces = make()
        _cases["rest/" + name] = (verts, faces, np.zeros((len(verts), 3)), None)
        _, _, targets, _, _ = wr.solver_case((verts, faces))
        _cases["noisy/" + name] = (verts, faces, widen(targets) - widen(verts), None)
    for name in ("odd_mesh", "flat", "strip2", "template"):
        verts, faces = MESHES[name]()
        for a, axis in enumerate(AXES):
            for angle in ANGLES:
                R = rotation_about(axis, angle)
                _cases[f"rigid/{name}/{a}/{angle:g}"] = (verts, faces, rigid_displacement(verts, R, (0.25, -0.5, 0.125)), R)
    verts, faces = MESHES["odd_mesh"]()
    mirror = np.zeros((len(verts), 3))
    mirror[:, 0] = -2.0 * widen(verts)[:, 0]
    _cases["mirrored/odd_mesh"] = (verts, faces, mirror, None)
    verts, faces = flat()
    mirror = np.zeros((len(verts), 3))
    mirror[:, 1] = -2.0 * widen(verts)[:, 1]
    _cases["mirrored/flat"] = (verts, faces, mirror, None)
    verts, faces, targets, _, _ = wr.solver_case("odd_mesh")
    for scale in (1e-6, 1e6):
        sv = (widen(verts) * scale).astype(np.float32)
        _cases[f"scaled/{scale:g}"] = (sv, faces, (widen(targets) - widen(verts)) * scale, None)
    linked = np.flatnonzero(np.diff(wr.adjacency(faces, len(verts))["offsets"]) > 0)
    for k, value in enumerate((np.nan, np.inf, -np.inf)):
        d = widen(targets) - widen(verts)
        d[linked[k + 1], k] = value
        _cases[f"non_finite/{k}"] = (verts, faces, d, None)
    return _cases


# ---- the scenes and conditions of the two claims (the CPU test applies them to the restatement, the GPU test to the GPU's own result) -------
RIGID = (rotation_about((1.0, 2.0, 2.0), 60.0), np.array([0.3, -0.2, 0.5]))


def deform_scene(which):
    """(verts, faces, handles, the rigidly moved patch [V,3] float64) of the 9 x 9 patch with its 32 border vertices or five vertices as
    handles of weight 1 under a rotation by 60 degrees about (1, 2, 2) / 3 plus a translation."""
    verts, faces = grid_patch(9)
    index = border_of(9) if which == "border" else np.array([0, 8, 72, 80, 40])
    truth = widen(verts) @ RIGID[0].T + RIGID[1]
    return verts, faces, (index, truth[index].astype(np.float32), 1.0), truth


def deform_condition(out, verts, faces, handles, truth, warped_to):
    """The deform condition on a result (the restatement's or the GPU's): at most 1e-3 from the rigidly moved patch and at least 100 times
    closer than one solve with the displacement regulariser."""
    err = float(np.linalg.norm(widen(np.asarray(out["verts"])) - truth, axis=1).max())
    base = float(np.linalg.norm(widen(np.asarray(warped_to)) - truth, axis=1).max())
    print("deform: max distance from the rigid motion", err, "warp_to", base, "ratio", base / err, "max |R - truth|",
          float(np.abs(np.asarray(out["rotations"]) - RIGID[0]).max()))
    return err <= 1e-3 and 100.0 * err <= base


def warp_to_with_handles(verts, faces, handles, truth):
    index, pos, _ = handles
    weight, targets = np.zeros(len(verts)), truth.astype(np.float32)
    weight[index] = 1.0
    targets[index] = pos
    return wr.warp_to(verts, faces, targets, weight, stiffness=1.0)[0]


def edge_change(before, after, faces):
    """The rms relative change of the edge lengths."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    l0, l1 = (np.linalg.norm(widen(np.asarray(v))[e[:, 0]] - widen(np.asarray(v))[e[:, 1]], axis=1) for v in (before, after))
    return float(np.sqrt((((l1 - l0) / l0) ** 2).mean()))


def rotated_template():
    tv, tf, pv, pf = wr.scene("patch")
    return (widen(tv) @ rotation_about((1.0, 2.0, 2.0), 15.0).T).astype(np.float32), tf, pv, pf


def warp_condition(results, verts, faces):
    """The warp condition on {"displacement": result, "arap": result}: the edge lengths change by at most 0.75 of the displacement model's
    and at least as many vertices are kept in the last iteration."""
    change = {m: edge_change(verts, r["verts"], faces) for m, r in results.items()}
    used = {m: r["history"][-1]["used"] for m, r in results.items()}
    print("warp: rms relative edge-length change", change, "kept", used, "residual rms", {m: r["history"][-1]["rms"] for m, r in results.items()})
    return change["arap"] <= 0.75 * change["displacement"] and used["arap"] >= used["displacement"]
