"""NumPy float32 restatement of the geometry export (include/mofanerf_hip.h, mofa_grid_points / mofa_iso_count / mofa_iso_emit): the same
grid formula, edge ids, vertex and face order, orientation and arithmetic, vectorised.  Test code, not product: the GPU output must equal
it exactly (faces equal, vertices bit for bit)."""
import numpy as np

DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], dtype=np.int64)   # +x +y +z +x+y +x+z +y+z +x+y+z
DIR_OF_OFFSET = np.array([-1, 0, 1, 3, 2, 4, 5, 6])          # (dx + 2 dy + 4 dz) -> direction
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
PERM_SIGN = [1, -1, -1, 1, 1, -1]
LONE_REST = np.array([(1, 2, 3), (0, 3, 2), (0, 1, 3), (0, 2, 1)])


def axis_coords(n, lo, step):
    """lo + (float)i * step, multiply and add rounded separately in float32."""
    return np.float32(lo) + np.arange(n).astype(np.float32) * np.float32(step)


def grid_points(res, lo, step):
    """[nx*ny*nz, 3] float32 in flat index order idx = (i*ny + j)*nz + k."""
    ax = [axis_coords(n, lo[a], step[a]) for a, n in enumerate(res)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X, Y, Z], -1).reshape(-1, 3)


def tet_corners(t):
    a, b, c = PERMS[t]
    c1 = 1 << a
    c2 = c1 | (1 << b)
    return [0, c1, c2, c2 | (1 << c)]


def marching_tets(grid, level, lo, step):
    """(verts [V,3] float32, faces [F,3] int32) of {grid >= level} — see the header for the rules."""
    g = np.asarray(grid, dtype=np.float32)
    nx, ny, nz = g.shape
    level = np.float32(level)
    inside = g >= level                                          # (NaN: False)
    flags = np.zeros((nx, ny, nz, 7), dtype=bool)
    for d, (dx, dy, dz) in enumerate(DIRS):
        flags[:nx - dx, :ny - dy, :nz - dz, d] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    flat = flags.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - flat                 # exclusive scan: vertex ids in increasing edge_id
    eid = np.nonzero(flat)[0]
    idx, d = eid // 7, eid % 7
    i, j, k = idx // (ny * nz), (idx // nz) % ny, idx % nz
    i2, j2, k2 = i + DIRS[d, 0], j + DIRS[d, 1], k + DIRS[d, 2]
    sa, sb = g[i, j, k], g[i2, j2, k2]
    t = (level - sa) / (sb - sa)
    ax = [axis_coords(n, lo[a], step[a]) for a, n in enumerate((nx, ny, nz))]
    verts = np.empty((len(eid), 3), dtype=np.float32)
    for a, (lo_i, hi_i) in enumerate(((i, i2), (j, j2), (k, k2))):
        pa, pb = ax[a][lo_i], ax[a][hi_i]
        verts[:, a] = pa + t * (pb - pa)

    # faces: every cell (C order), its 6 tets in permutation order, up to 2 triangles each
    ci, cj, ck = [q.reshape(-1) for q in np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")]
    n_cells = ci.size
    corner_idx = np.stack([((ci + (b & 1)) * ny + cj + ((b >> 1) & 1)) * nz + ck + (b >> 2) for b in range(8)], 1)
    corner_in = inside.reshape(-1)[corner_idx]
    tris = np.zeros((n_cells, 6, 2, 3), dtype=np.int64)
    valid = np.zeros((n_cells, 6, 2), dtype=bool)
    rows = np.arange(n_cells)
    for tt in range(6):
        cc = tet_corners(tt)
        ins = corner_in[:, cc].astype(np.int64)
        n_in = ins.sum(1)
        ev = np.zeros((n_cells, 4, 4), dtype=np.int64)           # vertex id of tet edge (u, w)
        for u in range(4):
            for w in range(u + 1, 4):
                e = 7 * corner_idx[:, cc[u]] + DIR_OF_OFFSET[cc[w] ^ cc[u]]
                ev[:, u, w] = ev[:, w, u] = vid[e]
        vv = lambda u, w: ev[rows, u, w]
        tri = np.zeros((n_cells, 2, 3), dtype=np.int64)
        # one corner alone on its side
        lone = np.where(n_in == 1, np.argmax(ins, 1), np.argmin(ins, 1))
        rest = LONE_REST[lone]
        one = n_in == 1
        tri[:, 0, 0] = vv(lone, rest[:, 0])
        tri[:, 0, 1] = vv(lone, np.where(one, rest[:, 1], rest[:, 2]))
        tri[:, 0, 2] = vv(lone, np.where(one, rest[:, 2], rest[:, 1]))
        # two and two: inside (p < q), outside (u < w), (p, q, u, w) made even by swapping u, w
        order_in = np.argsort(-ins, 1, kind="stable")           # inside corners first, each side in increasing order
        p, q, u, w = order_in[:, 0], order_in[:, 1], order_in[:, 2], order_in[:, 3]
        perm = np.stack([p, q, u, w], 1)
        inv = sum((perm[:, a] > perm[:, b]).astype(np.int64) for a in range(4) for b in range(a + 1, 4))
        odd = (inv & 1) == 1
        u, w = np.where(odd, w, u), np.where(odd, u, w)
        two = n_in == 2
        pu, pw, qw, qu = vv(p, u), vv(p, w), vv(q, w), vv(q, u)
        tri[two, 0] = np.stack([pu, pw, qw], 1)[two]
        tri[two, 1] = np.stack([pu, qw, qu], 1)[two]
        if PERM_SIGN[tt] < 0:
            tri = tri[:, :, [0, 2, 1]]
        tris[:, tt] = tri
        valid[:, tt, 0] = (n_in > 0) & (n_in < 4)
        valid[:, tt, 1] = two
    faces = tris.reshape(-1, 3)[valid.reshape(-1)]
    return verts, faces.astype(np.int32)


# ---- mesh properties (tests) --------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def is_closed_oriented_manifold(faces):
    """Every undirected edge lies in exactly two faces, used once in each direction."""
    e = directed_edges(faces)
    if len(e) == 0:
        return True
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rkey = e[:, 1] * (1 << 32) + e[:, 0]
    if len(np.unique(key)) != len(key):
        return False                                              # a directed edge used twice: inconsistent orientation / non-manifold
    return bool(np.isin(rkey, key).all())


def euler_characteristic(verts, faces):
    F = len(faces)
    E = len(directed_edges(faces)) // 2
    used = len(np.unique(np.asarray(faces).reshape(-1)))
    assert used == len(verts), "unreferenced vertices"
    return len(verts) - E + F


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- analytic fields (float32 on the grid of grid_points) ---------------------------------------------------------------------------
def field(name, res, lo, step):
    p = grid_points(res, lo, step).astype(np.float64)
    if name == "sphere":
        s = 0.6 - np.linalg.norm(p, axis=1)
    elif name == "torus":
        s = 0.2 - np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.55) ** 2 + p[:, 2] ** 2)
    elif name == "two_spheres":
        c = np.array([0.45, 0.0, 0.0])
        s = np.maximum(0.3 - np.linalg.norm(p - c, axis=1), 0.3 - np.linalg.norm(p + c, axis=1))
    else:
        raise ValueError(name)
    return s.astype(np.float32).reshape(res)


def cube_grid(res, a=1.0):
    """lo / step of [-a, a]^3 sampled at res, as mofanerf_amd.mesh.grid_spec computes them (float32)."""
    lo = np.full(3, -a, dtype=np.float32)
    hi = np.full(3, a, dtype=np.float32)
    step = ((hi - lo) / (np.asarray(res, dtype=np.float32) - np.float32(1))).astype(np.float32)
    return lo, step
