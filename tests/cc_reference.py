"""NumPy restatement of the mesh components (include/mofanerf_hip.h, mofa_cc_*; mofanerf_amd.mesh.components / select_components /
keep_components): union-find labels, numbering by smallest vertex index, -1 for unreferenced vertices, fp64 statistics with the absolute
sums the tolerance needs, the selection rules, the compaction, and a synchronous emulation of the hook / compress passes with its pass
count.  Test code, not product.  ``mismatches`` / ``compaction_mismatches`` are THE comparisons: the GPU tests assert they return
nothing, the CPU tests show that they see every injected fault."""
import numpy as np

import mt_reference as mt

EPS = 2.0 ** -52


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
def edges_of(faces, only_ab=False):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return f[:, [0, 1]] if only_ab else np.concatenate([f[:, [0, 1]], f[:, [1, 2]]], 0)


def union_find(V, edges, toward_larger=False):
    """root[v] of every vertex after joining the edges: the smallest (or, as a fault, the largest) vertex index of its component."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.asarray(edges).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            lo, hi = min(ra, rb), max(ra, rb)
            if toward_larger:
                parent[lo] = hi
            else:
                parent[hi] = lo
    return np.array([find(v) for v in range(V)], dtype=np.int64)


def dense_labels(V, faces, root):
    """(vertex_labels [V] int32, face_labels [F] int32, C): components numbered by the rank of their root among the referenced roots."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    referenced = np.zeros(V, dtype=bool)
    referenced[f.reshape(-1)] = True
    is_root = (root == np.arange(V)) & referenced
    rank = np.cumsum(is_root) - 1
    vertex_labels = np.where(referenced, rank[root], -1).astype(np.int32)
    return vertex_labels, vertex_labels[f[:, 0]].astype(np.int32), int(is_root.sum())


def face_terms(verts, faces):
    """[F,2] float64: 0.5 |(v1 - v0) x (v2 - v0)| and v0 . (v1 x v2) / 6, in the kernel's operation order (every operation rounded
    separately, sums left to right)."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p, q, r = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = q - p, r - p
    nx, ny, nz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    cx, cy, cz = q[:, 1] * r[:, 2] - q[:, 2] * r[:, 1], q[:, 2] * r[:, 0] - q[:, 0] * r[:, 2], q[:, 0] * r[:, 1] - q[:, 1] * r[:, 0]
    volume = ((p[:, 0] * cx + p[:, 1] * cy) + p[:, 2] * cz) / 6.0
    return np.stack([area, volume], 1)


def components(verts, faces, root=None):
    """What mesh.components returns, as NumPy arrays, plus ``abs_area`` / ``abs_volume`` (the sums of |term| per component)."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(verts)
    if V == 0 or len(f) == 0:
        z = np.zeros(0)
        return dict(n_components=0, vertex_labels=np.full(V, -1, dtype=np.int32), face_labels=np.full(len(f), -1, dtype=np.int32),
                    n_verts=z.astype(np.int64), n_faces=z.astype(np.int64), area=z, volume=z, abs_area=z, abs_volume=z,
                    bbox=np.zeros((0, 2, 3), dtype=np.float32), unreferenced=V)
    if root is None:
        root = union_find(V, edges_of(f))
    vl, fl, C = dense_labels(V, f, root)
    terms = face_terms(verts, f)
    ref = vl >= 0
    bbox = np.empty((C, 2, 3), dtype=np.float32)
    bbox[:, 0], bbox[:, 1] = np.inf, -np.inf
    np.minimum.at(bbox[:, 0], vl[ref], verts[ref])
    np.maximum.at(bbox[:, 1], vl[ref], verts[ref])
    s = lambda w: np.bincount(fl, weights=w, minlength=C)
    return dict(n_components=C, vertex_labels=vl, face_labels=fl, n_verts=np.bincount(vl[ref], minlength=C).astype(np.int64),
                n_faces=np.bincount(fl, minlength=C).astype(np.int64), area=s(terms[:, 0]), volume=s(terms[:, 1]),
                abs_area=s(np.abs(terms[:, 0])), abs_volume=s(np.abs(terms[:, 1])), bbox=bbox, unreferenced=int((~ref).sum()))


def same_partition(a, b):
    """Two label vectors describe one partition (labels < 0 are 'nobody' in both)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0):
        return False
    keep = a >= 0
    pairs = np.unique(np.stack([a[keep], b[keep]], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- the comparisons the GPU tests use --------------------------------------------------------------------------------------------------
def mismatches(got, want):
    """The keys of ``got`` (mesh.components' dict, tensors already on the host) that are not the reference's: labels, counts and boxes
    exactly, area and volume within (n_faces + 8) 2^-52 sum |term| — (n - 1) 2^-53 relative to the absolute sum bounds any summation
    order's error, twice that covers the reference's and the kernel's, the 8 their per-term roundings."""
    bad = [k for k in ("n_components", "unreferenced") if int(got[k]) != int(want[k])]
    for k, dt in (("vertex_labels", np.int32), ("face_labels", np.int32), ("n_verts", np.int64), ("n_faces", np.int64), ("bbox", np.float32)):
        g = np.asarray(got[k])
        if g.dtype != dt or g.shape != want[k].shape or not np.array_equal(g, want[k]):
            bad.append(k)
    for k in ("area", "volume"):
        g = np.asarray(got[k])
        bound = (want["n_faces"] + 8) * EPS * want["abs_" + k]
        if g.dtype != np.float64 or g.shape != want[k].shape or not (np.abs(g - want[k]) <= bound).all():
            bad.append(k)
    return bad


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def compaction_mismatches(got, want):
    """Indices of the elements of a (verts, faces, *per_vertex) tuple that differ from the reference's in dtype, shape or any bit."""
    if len(got) != len(want):
        return ["length"]
    return [i for i, (g, w) in enumerate(zip(got, want))
            if np.asarray(g).dtype != w.dtype or np.asarray(g).shape != w.shape or not np.array_equal(_bits(np.asarray(g)), _bits(w))]


# ---- selection and compaction -----------------------------------------------------------------------------------------------------------
def select(stats, keep):
    n_faces = stats["n_faces"]
    if isinstance(keep, str):
        assert keep == "largest"
        mask = np.zeros(stats["n_components"], dtype=bool)
        if len(mask):
            mask[int(np.flatnonzero(n_faces == n_faces.max())[0])] = True
        return mask
    if callable(keep):
        return np.asarray(keep(stats), dtype=bool)
    if isinstance(keep, (int, np.integer)):
        return n_faces >= keep
    return np.asarray(keep, dtype=bool)


def compact(verts, faces, stats, mask, *per_vertex):
    """(verts, faces, *per_vertex) of the kept components: vertices in old order, faces in old order with remapped indices."""
    verts, faces = np.asarray(verts), np.asarray(faces).reshape(-1, 3)
    vl, fl = stats["vertex_labels"], stats["face_labels"]
    if stats["n_components"] == 0:
        return (verts[:0], faces[:0]) + tuple(np.asarray(p)[:0] for p in per_vertex)
    vkeep = (vl >= 0) & mask[np.maximum(vl, 0)]
    vmap = np.where(vkeep, np.cumsum(vkeep) - 1, -1).astype(np.int32)
    return (verts[vkeep], vmap[faces[mask[fl]]].astype(np.int32).reshape(-1, 3)) + tuple(np.asarray(p)[vkeep] for p in per_vertex)


# ---- the passes, emulated synchronously -------------------------------------------------------------------------------------------------
def _roots(parent):
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            return parent
        parent = nxt


def emulate(V, faces, max_passes=64, only_ab=False, toward_larger=False):
    """(parent, passes): hook (every edge reads the roots of the pass's start, the writes combine as atomicMin does) then compress, until
    a pass changes nothing; ``passes`` counts that last pass too, as mesh.components does.  The two faults are the injected ones."""
    e = edges_of(faces, only_ab)
    parent = np.arange(V, dtype=np.int64)
    passes = 0
    while passes < max_passes:
        root = _roots(parent)
        ra, rb = root[e[:, 0]], root[e[:, 1]]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        parent = parent.copy()
        if toward_larger:
            np.maximum.at(parent, lo, hi)
        else:
            np.minimum.at(parent, hi, lo)
        parent = _roots(parent)
        passes += 1
        if not (ra != rb).any():
            break
    return parent, passes


# ---- test meshes ------------------------------------------------------------------------------------------------------------------------
FIELDS = (("sphere", (48, 64, 40)), ("two_spheres", (81, 40, 44)), ("torus", (70, 56, 33)))      # mt_reference fields on (-1, 1)^3, level 0
STRIPS = (3, 63, 64, 65, 255, 256, 257, 1025, 100003)
_cache = {}


def field_mesh(name, res):
    """(verts, faces) of mt_reference's field at level 0 on (-1, 1)^3 (computed once)."""
    if (name, res) not in _cache:
        lo, step = mt.cube_grid(res)
        _cache[name, res] = mt.marching_tets(mt.field(name, res, lo, step), 0.0, lo, step) + (lo, step)
    return _cache[name, res]


def shell_field(res, r1=0.35, r2=0.7):
    """float32 grid on (-1, 1)^3 that is >= 0 exactly in the shell r1 <= |p| <= r2: an outer surface and a cavity."""
    lo, step = mt.cube_grid(res)
    r = np.linalg.norm(mt.grid_points(res, lo, step).astype(np.float64), axis=1)
    return np.minimum(r2 - r, r - r1).astype(np.float32).reshape(res), lo, step


def permuted(verts, faces, seed):
    """The same mesh with randomly permuted vertex numbering: vertex v becomes perm[v]."""
    perm = np.random.default_rng(seed).permutation(len(verts))
    out = np.empty_like(verts)
    out[perm] = verts
    return out, perm[np.asarray(faces, dtype=np.int64)].astype(np.int32), perm


def strip(V, seed, numbering="random"):
    """A triangle strip over V vertices (faces (i, i+1, i+2), every other one flipped) with random / identity / reversed / zig-zag
    numbering and random float32 coordinates: one component whose label has to travel V - 1 links."""
    rng = np.random.default_rng(seed)
    i = np.arange(V - 2)
    faces = np.stack([i, i + 1 + (i & 1), i + 2 - (i & 1)], 1)
    if numbering == "random":
        perm = rng.permutation(V)
    elif numbering == "identity":
        perm = np.arange(V)
    elif numbering == "reversed":
        perm = np.arange(V)[::-1].copy()
    else:                                                         # zig-zag: 0, V-1, 1, V-2, ...
        perm = np.empty(V, dtype=np.int64)
        perm[0::2], perm[1::2] = np.arange((V + 1) // 2), V - 1 - np.arange(V // 2)
    return rng.standard_normal((V, 3)).astype(np.float32), perm[faces].astype(np.int32)


def bow_tie():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (-1, 0, 1), (0, -1, 1)], dtype=np.float32)
    return verts, np.array([(2, 0, 1), (3, 2, 4)], dtype=np.int32)


def odd_mesh():
    """Degenerate faces, unreferenced vertices and interleaved components: {1, 8, 9} (smallest vertex 1, largest 9) joined only through
    the degenerate (9, 9, 1) and (8, 1, 1); {3, 4, 6}; {5, 7, 11, 12}; vertices 0, 2, 10 and 13 belong to no face."""
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((14, 3)).astype(np.float32)
    faces = np.array([(9, 9, 1), (4, 6, 3), (12, 5, 7), (8, 1, 1), (11, 7, 12), (6, 4, 3), (7, 7, 7)], dtype=np.int32)
    return verts, faces
