"""NumPy restatement of the mesh smoothing (mofanerf_amd/csrc/mofa_smooth.hip, mesh.vertex_adjacency, mesh.smooth): the adjacency from the
stably sorted half-edge entries, the boundary, the corner cotangents, the clamped edge weights, the step and the Taubin loop, in the
arithmetic include/mofanerf_hip.h states: fp64 on the fp32 coordinates widened, every operation a separate NumPy call (so rounded
separately), every sum sequential in the stated order (neighbour k of every vertex is added in round k; a round touches every vertex at most
once).  ``fault=`` injects one deviation at a time (FAULTS); tests/test_smooth_reference_cpu.py shows that each changes an output bit on a
mesh the GPU tests use.  The meshes of both test files live here too."""
import numpy as np

import mt_reference as mt

FAULTS = ("no_dedup", "reversed_order", "self_loops", "no_division", "skip_mu", "in_place", "fp32_accumulate", "wrong_corner", "no_clamp",
          "boundary_free")
STAT_INTS = ("passes", "n_pinned", "n_boundary", "n_isolated", "degree_max", "edges_nonmanifold", "flat_corners", "negative_weights", "zero_weight")


def adjacency(faces, V, fault=None):
    """mesh.vertex_adjacency's dict (NumPy) plus ``perm`` / ``seg`` (the sorted entries and the runs the edge weights sum over)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= V):
        raise ValueError("face index outside [0, V)")
    a, b = f[:, [1, 2, 0]], f[:, [2, 0, 1]]                              # corner c: the edge opposite to it
    i, j = np.stack([a, b], -1).reshape(-1), np.stack([b, a], -1).reshape(-1)         # entry e = 2 (3 f + c) + dir
    entry = np.flatnonzero(i != j)
    key = (i[entry] << 31) | j[entry]
    order = np.argsort(key, kind="stable")
    pair, run = np.unique(key[order], return_counts=True)
    pi, pj = pair >> 31, pair & (2 ** 31 - 1)
    boundary = np.zeros(V, dtype=bool)
    boundary[pi[run == 1]] = True
    nonmanifold = int(((run > 2) & (pi < pj)).sum())
    if fault == "self_loops":                                            # the entries (a, a) stay: a vertex becomes its own neighbour
        entry = np.arange(len(i))
        key = (i << 31) | j
        order = np.argsort(key, kind="stable")
        pair, run = np.unique(key[order], return_counts=True)
    if fault == "no_dedup":                                              # every entry is a pair of its own
        pair, run = key[order], np.ones(len(order), dtype=np.int64)
    pi, pj = pair >> 31, pair & (2 ** 31 - 1)
    degree = np.bincount(pi, minlength=V).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(degree)]).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(run)]).astype(np.int64)
    perm = entry[order].astype(np.int64)
    if fault == "reversed_order":                                        # each vertex's neighbours descend
        rev = np.concatenate([np.arange(offsets[v + 1] - 1, offsets[v] - 1, -1) for v in range(V)]).astype(np.int64) if len(pair) else np.zeros(0, np.int64)
        pj, run = pj[rev], run[rev]
        perm = np.concatenate([perm[seg[p]:seg[p + 1]] for p in rev]) if len(rev) else perm
        seg = np.concatenate([[0], np.cumsum(run)]).astype(np.int64)
    return {"offsets": offsets, "neighbours": pj.astype(np.int32), "degree_max": int(degree.max()) if V else 0, "boundary": boundary,
            "edges_nonmanifold": nonmanifold, "perm": perm, "seg": seg}


def corner_cots(verts, faces, fault=None):
    """(cots [F,3] float64, flat_corners)."""
    x, f = np.asarray(verts, dtype=np.float32).astype(np.float64), np.asarray(faces, dtype=np.int64)
    cots, flat = np.zeros((len(f), 3)), 0
    for c in range(3):
        o, a, b = x[f[:, c]], x[f[:, (c + 1) % 3]], x[f[:, (c + 2) % 3]]
        u, v = a - o, b - o
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        n = np.sqrt((cx * cx + cy * cy) + cz * cz)
        d = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
        ok = (n != 0) & np.isfinite(n)
        with np.errstate(all="ignore"):
            cots[:, c] = np.where(ok, d / np.where(ok, n, 1.0), 0.0)
        flat += int((~ok).sum())
    if fault == "wrong_corner":                                          # the cotangent at a, not at the apex opposite the edge
        cots = cots[:, [1, 2, 0]]
    return cots, flat


def edge_weights(cots, adj, fault=None):
    """(weights [E] float64, negative_weights): the sequential sum of 0.5 cot over each pair's run, then the clamp."""
    perm, seg = adj["perm"], adj["seg"]
    run, flat = np.diff(seg), cots.reshape(-1)
    w = np.zeros(len(run))
    for k in range(int(run.max()) if len(run) else 0):
        m = np.flatnonzero(run > k)
        w[m] = w[m] + 0.5 * flat[perm[seg[m] + k] // 2]
    negative = w < 0
    if fault != "no_clamp":
        w = np.where(negative, 0.0, w)
    return w, int(negative.sum())


def step(x32, adj, w, pin, factor, fault=None):
    """(out [V,3] float32, zero_weight) of one pass."""
    acc = np.float32 if fault == "fp32_accumulate" else np.float64
    off, nbr = adj["offsets"], adj["neighbours"].astype(np.int64)
    deg = np.diff(off)
    V = len(x32)
    if fault == "in_place":                                              # vertex i reads the neighbours below it already moved
        cur, zero = x32.copy(), 0
        for i in np.flatnonzero((deg > 0) & ~pin):
            xi, s, sw = cur[i].astype(acc), np.zeros(3, acc), acc(0)
            for k in range(off[i], off[i + 1]):
                d = cur[nbr[k]].astype(acc) - xi
                if w is None:
                    s = s + d
                else:
                    s, sw = s + acc(w[k]) * d, sw + acc(w[k])
            if w is None:
                sw = acc(deg[i])
            if not sw > 0:
                zero += 1
                continue
            cur[i] = (xi + acc(factor) * (s / sw)).astype(np.float32)
        return cur, zero
    x = x32.astype(acc)
    s, sw = np.zeros((V, 3), acc), np.zeros(V, acc)
    for k in range(int(deg.max()) if V else 0):
        m = np.flatnonzero(deg > k)
        idx = off[m] + k
        d = x[nbr[idx]] - x[m]
        if w is None:
            s[m] = s[m] + d
        else:
            wk = w[idx].astype(acc)
            s[m] = s[m] + wk[:, None] * d
            sw[m] = sw[m] + wk
    if w is None:
        sw = deg.astype(acc)
    move = (deg > 0) & ~pin
    zero = move & ~(sw > 0)
    move &= ~zero
    out = x32.copy()
    with np.errstate(all="ignore"):
        L = s[move] if fault == "no_division" else s[move] / sw[move][:, None]
        out[move] = (x[move] + acc(factor) * L).astype(np.float32)
    return out, int(zero.sum())


def displacement(out, verts):
    d = np.asarray(out, np.float32).astype(np.float64) - np.asarray(verts, np.float32).astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, weights="uniform", boundary="fixed", pinned=None, fault=None):
    """mesh.smooth's ``(verts', stats)`` in NumPy (the parameters are taken as valid)."""
    verts, faces = np.ascontiguousarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = len(verts), len(faces)
    stats = dict.fromkeys(STAT_INTS, 0)
    stats.update(displacement=np.zeros(V, np.float32), max_displacement=0.0)
    if iterations == 0 or V == 0 or F == 0:
        return verts.copy(), stats
    adj = adjacency(faces, V, fault)
    ref = np.zeros(V, dtype=bool)
    ref[faces.reshape(-1)] = True
    if not np.isfinite(verts[ref]).all():
        raise ValueError("non-finite referenced vertex")
    pin = adj["boundary"].copy() if boundary == "fixed" and fault != "boundary_free" else np.zeros(V, dtype=bool)
    if pinned is not None:
        pin |= np.asarray(pinned, dtype=bool)
    deg = np.diff(adj["offsets"])
    stats.update(n_pinned=int(pin.sum()), n_boundary=int(adj["boundary"].sum()), n_isolated=int((deg == 0).sum()), degree_max=adj["degree_max"],
                 edges_nonmanifold=adj["edges_nonmanifold"])
    if len(adj["neighbours"]) == 0:
        return verts.copy(), stats
    w = None
    if weights == "cotangent":
        cots, stats["flat_corners"] = corner_cots(verts, faces, fault)
        w, stats["negative_weights"] = edge_weights(cots, adj, fault)
    factors = [lam] if mu is None or fault == "skip_mu" else [lam, mu]
    cur = verts
    for _ in range(iterations):
        for factor in factors:
            cur, stats["zero_weight"] = step(cur, adj, w, pin, factor, fault)
    stats["passes"] = iterations * (1 if mu is None else 2)
    stats["displacement"] = displacement(cur, verts)
    stats["max_displacement"] = float(stats["displacement"].max())
    return cur, stats


def mismatches(got, want):
    """What differs between two ``(verts, stats)`` results, as a list of words: the vertices bit for bit, the integers exactly, the
    displacement within 1 ulp (fp32)."""
    (gv, gs), (wv, ws) = got, want
    gv, wv = np.asarray(gv), np.asarray(wv)
    out = []
    if gv.dtype != np.float32 or gv.shape != wv.shape or not np.array_equal(gv.view(np.uint32), wv.view(np.uint32)):
        out.append("verts")
    out += [k for k in STAT_INTS if int(gs[k]) != int(ws[k])]
    gd, wd = np.asarray(gs["displacement"]), np.asarray(ws["displacement"])
    if gd.dtype != np.float32 or gd.shape != wd.shape or not (np.abs(gd.astype(np.float64) - wd) <= np.spacing(wd)).all():
        out.append("displacement")
    if not abs(float(gs["max_displacement"]) - float(ws["max_displacement"])) <= float(np.spacing(np.float32(ws["max_displacement"]))):
        out.append("max_displacement")
    return out


def radial_std(verts):
    return float(np.linalg.norm(np.asarray(verts, dtype=np.float64), axis=1).std())


# ---- the meshes ----------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    """The regular tetrahedron on four corners of the cube [-1, 1]^3, normals outward."""
    verts = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], dtype=np.float32)
    return verts, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], dtype=np.int32)


def octahedron():
    verts = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float32)
    return verts, np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=np.int32)


def grid_patch(nx=9, ny=9, seed=0, noise=0.1):
    """An open plane patch of nx x ny vertices at unit spacing with z-noise from a fixed seed, two faces per cell."""
    rng = np.random.default_rng(seed)
    I, J = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    verts = np.stack([I.reshape(-1), J.reshape(-1), noise * rng.standard_normal(nx * ny)], -1).astype(np.float32)
    v = lambda i, j: i * ny + j
    faces = [t for i in range(nx - 1) for j in range(ny - 1)
             for t in ((v(i, j), v(i + 1, j), v(i + 1, j + 1)), (v(i, j), v(i + 1, j + 1), v(i, j + 1)))]
    return verts, np.array(faces, dtype=np.int32)


def fan(n=300, seed=1):
    """One hub (vertex 0) of degree n above a noisy rim of n vertices: a closed fan, open at the rim."""
    rng = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), np.sin(t), 0.05 * rng.standard_normal(n)], -1)
    verts = np.concatenate([[(0.03, -0.02, 0.5)], rim]).astype(np.float32)
    return verts, np.array([(0, 1 + k, 1 + (k + 1) % n) for k in range(n)], dtype=np.int32)


_spheres = {}


def mt_sphere(res=17, binary=True):
    """The marching-tetrahedra mesh of the ball of radius 0.6 on [-1, 1]^3 sampled at res^3: of the field 0.6 - |p| at level 0, or
    (``binary``) of its indicator at level 0.5, whose vertices sit at edge midpoints: staircase noise one cell high."""
    if (res, binary) not in _spheres:
        lo, step = mt.cube_grid((res,) * 3)
        grid = mt.field("sphere", (res,) * 3, lo, step).reshape((res,) * 3)
        _spheres[res, binary] = mt.marching_tets((grid > 0).astype(np.float32), 0.5, lo, step) if binary else mt.marching_tets(grid, 0.0, lo, step)
    v, f = _spheres[res, binary]
    return v.copy(), f.copy()


def odd_mesh():
    """A tetrahedron with its first face duplicated, an unreferenced vertex (4), a degenerate face (0, 0, 5) that makes 5 a neighbour of
    0, and a vertex (6) only the face (6, 6, 6) references: no neighbours."""
    verts, faces = tetrahedron()
    verts = np.concatenate([verts + np.float32(0.125) * np.arange(12, dtype=np.float32).reshape(4, 3) / 12,
                            [(5, 5, 5), (2, 2.5, 3), (-3, 0, 1)]]).astype(np.float32)
    return verts, np.concatenate([faces, faces[:1], [(0, 0, 5), (6, 6, 6)]]).astype(np.int32)


def strip(V=257, seed=2):
    """A triangle strip of V vertices in two rows with z-noise (every vertex is on the boundary): V = 257 crosses one 256-thread block."""
    rng = np.random.default_rng(seed)
    k = np.arange(V)
    verts = np.stack([0.5 * k, k % 2, 0.2 * rng.standard_normal(V)], -1).astype(np.float32)
    return verts, np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(V - 2)], dtype=np.int32)


def wide_fan():
    """A fan of 8 rim vertices whose heights span 2^40: the fp64 sums of fp32 differences, exact on every ordinary mesh (29 spare bits),
    round here, so the order of the neighbours shows in the result."""
    z = np.array([0.0, 1.0001, 2.0 ** 40, -2.0 ** 40, 0.3, -0.7, 2.0 ** 38, 0.123456, -2.0 ** 38])
    t = 2 * np.pi * np.arange(8) / 8
    verts = np.stack([np.concatenate([[0.0], np.cos(t)]), np.concatenate([[0.0], np.sin(t)]), z], -1).astype(np.float32)
    return verts, np.array([(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)], dtype=np.int32)


MESHES = (("tetrahedron", tetrahedron), ("wide_fan", wide_fan), ("octahedron", octahedron), ("grid_patch", grid_patch), ("fan", fan),
          ("mt_sphere_binary", lambda: mt_sphere(17, True)), ("mt_sphere", lambda: mt_sphere(9, False)), ("odd_mesh", odd_mesh), ("strip", strip))
