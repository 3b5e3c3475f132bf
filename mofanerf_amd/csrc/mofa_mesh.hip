// Geometry export (gfx950): the sample points of a regular grid, and the iso-surface of a density grid as a triangle mesh by marching
// tetrahedra on the Freudenthal split.  Deterministic with no atomics: vertex and face slots come from 64-bit exclusive scans of
// per-edge / per-cell counts, so the output is the same bits on every run.
//
//   grid points     idx = (i * ny + j) * nz + k (C order, z fastest);  x = lo_x + (float)i * step_x (separately rounded)
//   tets            cell (i,j,k) -> 6 tets {0, e_a, e_a + e_b, e_a + e_b + e_c}, one per axis permutation (a,b,c) in lexicographic order
//   edges           7 lattice directions +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z;  edge_id = 7 idx + dir, owned by its lower endpoint
//   inside          sigma >= level (NaN is outside); an edge carries a vertex when its two ends differ
//   vertex          t = (level - s_a) / (s_b - s_a), p = p_a + t (p_b - p_a), every operation separately rounded, a = lower endpoint
//   order           vertices by edge_id; faces by cell, then tet, then triangle; normals (v1 - v0) x (v2 - v0) point toward lower sigma
//
// Kernels: k_iso_edge_flags, k_iso_cell_counts (+ the scans and k_iso_totals: mofa_iso_count), k_iso_vertices, k_iso_faces (mofa_iso_emit),
// k_iso_edge_ids (mofa_iso_edge_ids: each vertex's edge, for the refinement in mofa_refine.hip).
#include <math.h>

#include "mofa_common.h"
#include "mofa_lattice.h"

namespace mofa {
namespace {

constexpr int kScanItems = 8;                       // elements per thread of one scan tile
constexpr int kScanTile = 256 * kScanItems;         // elements per workgroup
constexpr long long kIsoMaxEdges = 1ll << 31;       // 7 nx ny nz must stay below this
constexpr long long kIsoMaxOut = 2147483647ll;      // V and F must fit int32 face indices

// (grid_coord, inside and the direction tables kDirDx / kDirDy / kDirDz: mofa_lattice.h)
// offset (dx + 2 dy + 4 dz) of a tet edge -> lattice direction 0..6 (+x, +y, +z, +x+y, +x+z, +y+z, +x+y+z)
__device__ __constant__ int kDirOfOffset[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// the 6 axis permutations (a,b,c) in lexicographic order, and the sign of each (the orientation of its tet)
__device__ __constant__ int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__device__ __constant__ int kPermSign[6] = {1, -1, -1, 1, 1, -1};
// one inside (or one outside) corner i: the other three in the order (j,k,l) that makes (i,j,k,l) an even permutation of (0,1,2,3)
__device__ __constant__ int kLoneRest[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};

// the four corners of tet `t` of a cell as lattice offsets (bit 0: x, bit 1: y, bit 2: z)
__device__ __forceinline__ void tet_corners(int t, int (&c)[4]) {
    c[0] = 0;
    c[1] = c[0] | (1 << kPerm[t][0]);
    c[2] = c[1] | (1 << kPerm[t][1]);
    c[3] = c[2] | (1 << kPerm[t][2]);
}

__device__ __forceinline__ int tet_triangles(int n_in) { return (n_in == 1 || n_in == 3) ? 1 : (n_in == 2 ? 2 : 0); }

// the triangles of tet `t` of a cell whose inside corners are the bits of `in`: up to 2, oriented (normals toward lower sigma); the
// vertex id of the tet edge between tet corners u and w is vid(lo, hi, dir): lo / hi the cell-corner offsets of its lower and upper end,
// dir its lattice direction.  Returns the number of triangles.
template <typename Vid>
__device__ __forceinline__ int tet_tris(unsigned in, int t, Vid vid_of, long long (&out)[2][3]) {
    int cc[4];
    tet_corners(t, cc);
    int ins[4], n_in = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) ins[u] = (int)((in >> cc[u]) & 1), n_in += ins[u];
    if (n_in == 0 || n_in == 4) return 0;
    // (the corners grow componentwise, so the lower end of the edge between u and w is min(u, w))
    auto vid = [&](int u, int w) -> long long {
        const int lo = u < w ? u : w, hi = u < w ? w : u;
        return vid_of(cc[lo], cc[hi], kDirOfOffset[cc[hi] ^ cc[lo]]);
    };
    long long tri[2][3];
    int n_tri;
    if (n_in != 2) {
        int lone = 0;                                   // the corner alone on its side
        for (int u = 0; u < 4; ++u)
            if (ins[u] == (n_in == 1 ? 1 : 0)) lone = u;
        const int* rest = kLoneRest[lone];
        // (lone, rest) even: the triangle's normal points away from `lone` — outward when it is the one inside corner
        tri[0][0] = vid(lone, rest[0]);
        tri[0][1] = vid(lone, n_in == 1 ? rest[1] : rest[2]);
        tri[0][2] = vid(lone, n_in == 1 ? rest[2] : rest[1]);
        n_tri = 1;
    } else {
        // inside pair (p, q), outside pair (u, w) with (p, q, u, w) even: the quad (pu, pw, qw, qu) faces the outside corners
        int p = -1, q = -1, u = -1, w = -1;
        for (int x = 0; x < 4; ++x) {
            if (ins[x]) (p < 0 ? p : q) = x;
            else (u < 0 ? u : w) = x;
        }
        // an odd (p, q, u, w) becomes even by swapping u and w
        const int perm[4] = {p, q, u, w};
        int inv = 0;
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b) inv += perm[a] > perm[b];
        if (inv & 1) { const int tmp = u; u = w; w = tmp; }
        const long long pu = vid(p, u), pw = vid(p, w), qw = vid(q, w), qu = vid(q, u);
        tri[0][0] = pu, tri[0][1] = pw, tri[0][2] = qw;
        tri[1][0] = pu, tri[1][1] = qw, tri[1][2] = qu;
        n_tri = 2;
    }
    const bool flip = kPermSign[t] < 0;                // a negatively oriented tet mirrors every normal
    for (int s = 0; s < n_tri; ++s) {
        out[s][0] = tri[s][0];
        out[s][1] = flip ? tri[s][2] : tri[s][1];
        out[s][2] = flip ? tri[s][1] : tri[s][2];
    }
    return n_tri;
}

__global__ __launch_bounds__(256) void k_grid_points(long long ny, long long nz, float lox, float loy, float loz, float sx, float sy, float sz,
                                                     long long first, long long n, float* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long long idx = first + t, i = idx / (ny * nz), r = idx - i * (ny * nz), j = r / nz, k = r - j * nz;
    pts[t * 3 + 0] = grid_coord(lox, sx, i);
    pts[t * 3 + 1] = grid_coord(loy, sy, j);
    pts[t * 3 + 2] = grid_coord(loz, sz, k);
}

// flags[7 idx + dir] = 1 where the edge lies in the grid and its two ends are on different sides of the level
__global__ __launch_bounds__(256) void k_iso_edge_flags(const float* __restrict__ grid, long long nx, long long ny, long long nz, float level,
                                                        unsigned char* __restrict__ flags) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= 7 * nx * ny * nz) return;
    const long long idx = e / 7;
    const int dir = (int)(e - idx * 7);
    const long long i = idx / (ny * nz), r = idx - i * (ny * nz), j = r / nz, k = r - j * nz;
    const long long i2 = i + kDirDx[dir], j2 = j + kDirDy[dir], k2 = k + kDirDz[dir];
    unsigned char f = 0;
    if (i2 < nx && j2 < ny && k2 < nz) f = inside(grid[idx], level) != inside(grid[(i2 * ny + j2) * nz + k2], level) ? 1 : 0;
    flags[e] = f;
}

// counts[cell] = triangles of the cell's six tets (0 .. 12)
__global__ __launch_bounds__(256) void k_iso_cell_counts(const float* __restrict__ grid, long long nx, long long ny, long long nz, float level,
                                                         unsigned char* __restrict__ counts) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long cy = ny - 1, cz = nz - 1;
    if (c >= (nx - 1) * cy * cz) return;
    const long long i = c / (cy * cz), r = c - i * (cy * cz), j = r / cz, k = r - j * cz;
    unsigned in = 0;                                   // bit b: corner b (bit 0 = +x, bit 1 = +y, bit 2 = +z) is inside
#pragma unroll
    for (int b = 0; b < 8; ++b)
        in |= (inside(grid[((i + (b & 1)) * ny + j + ((b >> 1) & 1)) * nz + k + (b >> 2)], level) ? 1u : 0u) << b;
    int n = 0;
    for (int t = 0; t < 6; ++t) {
        int cc[4];
        tet_corners(t, cc);
        n += tet_triangles((int)((in >> cc[0]) & 1) + (int)((in >> cc[1]) & 1) + (int)((in >> cc[2]) & 1) + (int)((in >> cc[3]) & 1));
    }
    counts[c] = (unsigned char)n;
}

// ---- 64-bit exclusive scan (three kernels, recursive over the tile sums; integer, so exact and reproducible) -------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_scan_tiles(const T* __restrict__ in, long long n, long long* __restrict__ out,
                                                    long long* __restrict__ tile_sums) {
    __shared__ long long part[256];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long v[kScanItems], s = 0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
        v[q] = base + q < n ? (long long)in[base + q] : 0;
        s += v[q];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {        // inclusive Hillis-Steele scan of the 256 thread sums
        const long long add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - s;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
        if (base + q < n) out[base + q] = run;
        run += v[q];
    }
    if (threadIdx.x == 255) tile_sums[blockIdx.x] = part[255];
}

__global__ __launch_bounds__(256) void k_scan_add(long long* __restrict__ out, long long n, const long long* __restrict__ tile_offsets) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] += tile_offsets[e / kScanTile];
}

// V and F from the scans' last elements: into the caller's counts and the workspace (where mofa_iso_emit's kernels look)
__global__ void k_iso_totals(const long long* __restrict__ escan, const unsigned char* __restrict__ eflags, long long n_edges,
                             const long long* __restrict__ cscan, const unsigned char* __restrict__ ccounts, long long n_cells,
                             long long* __restrict__ totals, long long* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    const long long V = escan[n_edges - 1] + eflags[n_edges - 1], F = cscan[n_cells - 1] + ccounts[n_cells - 1];
    totals[0] = V, totals[1] = F;
    counts[0] = V, counts[1] = F;
}

__global__ __launch_bounds__(256) void k_iso_vertices(const float* __restrict__ grid, long long nx, long long ny, long long nz, float level,
                                                      float lox, float loy, float loz, float sx, float sy, float sz,
                                                      const unsigned char* __restrict__ flags, const long long* __restrict__ escan,
                                                      const long long* __restrict__ totals, float* __restrict__ verts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= 7 * nx * ny * nz || !flags[e]) return;
    if (totals[0] > kIsoMaxOut || totals[1] > kIsoMaxOut) return;      // (refused: the host was told by the counts)
    const long long idx = e / 7;
    const int dir = (int)(e - idx * 7);
    const long long i = idx / (ny * nz), r = idx - i * (ny * nz), j = r / nz, k = r - j * nz;
    const long long i2 = i + kDirDx[dir], j2 = j + kDirDy[dir], k2 = k + kDirDz[dir];
    const float sa = grid[idx], sb = grid[(i2 * ny + j2) * nz + k2];
    const float t = __fdiv_rn(__fsub_rn(level, sa), __fsub_rn(sb, sa));
    const float pa[3] = {grid_coord(lox, sx, i), grid_coord(loy, sy, j), grid_coord(loz, sz, k)};
    const float pb[3] = {grid_coord(lox, sx, i2), grid_coord(loy, sy, j2), grid_coord(loz, sz, k2)};
    const long long v = escan[e];
#pragma unroll
    for (int a = 0; a < 3; ++a) verts[v * 3 + a] = __fadd_rn(pa[a], __fmul_rn(t, __fsub_rn(pb[a], pa[a])));
}

// edge_ids[v] = the edge of vertex v: the flagged edges compacted through their scan (k_iso_vertices' numbering)
__global__ __launch_bounds__(256) void k_iso_edge_ids(long long n_edges, const unsigned char* __restrict__ flags,
                                                      const long long* __restrict__ escan, const long long* __restrict__ totals,
                                                      int64_t* __restrict__ edge_ids) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges || !flags[e]) return;
    if (totals[0] > kIsoMaxOut || totals[1] > kIsoMaxOut) return;
    edge_ids[escan[e]] = e;
}

__global__ __launch_bounds__(256) void k_iso_faces(const float* __restrict__ grid, long long nx, long long ny, long long nz, float level,
                                                   const unsigned char* __restrict__ ccounts, const long long* __restrict__ cscan,
                                                   const long long* __restrict__ escan, const long long* __restrict__ totals,
                                                   int* __restrict__ faces) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long cy = ny - 1, cz = nz - 1;
    if (c >= (nx - 1) * cy * cz || !ccounts[c]) return;
    if (totals[0] > kIsoMaxOut || totals[1] > kIsoMaxOut) return;
    const long long i = c / (cy * cz), r = c - i * (cy * cz), j = r / cz, k = r - j * cz;
    long long idx[8];
    unsigned in = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        idx[b] = ((i + (b & 1)) * ny + j + ((b >> 1) & 1)) * nz + k + (b >> 2);
        in |= (inside(grid[idx[b]], level) ? 1u : 0u) << b;
    }
    long long f = cscan[c];
    for (int t = 0; t < 6; ++t) {
        long long tri[2][3];
        const int n_tri = tet_tris(in, t, [&](int lo, int, int dir) { return escan[7 * idx[lo] + dir]; }, tri);
        for (int s = 0; s < n_tri; ++s, ++f)
            for (int a = 0; a < 3; ++a) faces[f * 3 + a] = (int)tri[s][a];
    }
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

// elements of scan scratch (tile sums and their scans, every level) for an exclusive scan of n elements
long long scan_aux(long long n) {
    const long long nb = (n + kScanTile - 1) / kScanTile;
    return nb + (nb > 1 ? nb + scan_aux(nb) : 0);
}

// out[0..n) = exclusive prefix sums of in[0..n) (T = unsigned char or long long); aux: scan_aux(n) elements
template <typename T>
int scan_exclusive(const T* in, long long n, long long* out, long long* aux, hipStream_t st) {
    const long long nb = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_tiles<T>, dim3((unsigned)nb), dim3(256), 0, st, in, n, out, aux);
    if (nb > 1) {
        const int rc = scan_exclusive<long long>(aux, nb, aux + nb, aux + 2 * nb, st);
        if (rc != MOFA_OK) return rc;
        hipLaunchKernelGGL(k_scan_add, dim3(blocks_of(n)), dim3(256), 0, st, out, n, (const long long*)(aux + nb));
    }
    return check_launch("k_scan_tiles");
}

constexpr size_t kAlign = 256;
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// the workspace of one extraction: edge flags, their scan, cell triangle counts, their scan, the scans' scratch, V / F
struct IsoLayout {
    long long n_edges, n_cells;
    size_t eflags, escan, ccounts, cscan, aux, totals, bytes;
};
IsoLayout iso_layout(long long nx, long long ny, long long nz) {
    IsoLayout l{};
    l.n_edges = 7 * nx * ny * nz;
    l.n_cells = (nx - 1) * (ny - 1) * (nz - 1);
    const long long aux_e = scan_aux(l.n_edges), aux_c = scan_aux(l.n_cells);
    size_t o = 0;
    l.eflags = o, o = align_up(o + (size_t)l.n_edges);
    l.escan = o, o = align_up(o + (size_t)l.n_edges * 8);
    l.ccounts = o, o = align_up(o + (size_t)l.n_cells);
    l.cscan = o, o = align_up(o + (size_t)l.n_cells * 8);
    l.aux = o, o = align_up(o + (size_t)(aux_e > aux_c ? aux_e : aux_c) * 8);
    l.totals = o, o = align_up(o + 2 * 8);
    l.bytes = o;
    return l;
}

// a grid the extraction takes: >= 2 samples per axis and 7 nx ny nz < 2^31 (checked without overflow)
bool iso_grid_ok(long long nx, long long ny, long long nz) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    if (nx >= kIsoMaxEdges || ny >= kIsoMaxEdges || nz >= kIsoMaxEdges) return false;
    if (7 * nx * ny >= kIsoMaxEdges) return false;
    return 7 * nx * ny * nz < kIsoMaxEdges;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_ISO_GRID(what)                                                                                                               \
    MOFA_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, what ": the grid needs at least 2 samples per axis (got %lld x %lld x %lld)", (long long)nx, \
                 (long long)ny, (long long)nz);                                                                                           \
    MOFA_REQUIRE(iso_grid_ok(nx, ny, nz), what ": grid %lld x %lld x %lld is too large (7 nx ny nz must stay below 2^31)", (long long)nx,   \
                 (long long)ny, (long long)nz)

extern "C" {

// the scan, for the occupancy kernels' compaction (mofa_occ.hip): out[0..n) = exclusive prefix sums of the bytes in[0..n), aux of
// mofa_internal_scan_aux(n) elements
long long mofa_internal_scan_aux(long long n) { return scan_aux(n); }
int mofa_internal_scan_bytes(const unsigned char* in, long long n, long long* out, long long* aux, void* stream) {
    return scan_exclusive<unsigned char>(in, n, out, aux, (hipStream_t)stream);
}

int mofa_grid_points(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], int64_t first, int64_t n, float* pts,
                     void* stream) {
    MOFA_REQUIRE(lo && step && pts, "grid_points: null pointer");
    MOFA_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx < (1ll << 24) && ny < (1ll << 24) && nz < (1ll << 24) && nx * ny < (1ll << 40) &&
                     nx * ny * nz < (1ll << 48),
                 "grid_points: grid %lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);
    MOFA_REQUIRE(first >= 0 && n > 0 && first + n <= nx * ny * nz, "grid_points: points [%lld, %lld) of %lld", (long long)first,
                 (long long)(first + n), (long long)(nx * ny * nz));
    hipLaunchKernelGGL(k_grid_points, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, (long long)ny, (long long)nz, lo[0], lo[1], lo[2],
                       step[0], step[1], step[2], (long long)first, (long long)n, pts);
    return check_launch("k_grid_points");
}

size_t mofa_iso_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (!iso_grid_ok(nx, ny, nz)) return 0;
    return iso_layout(nx, ny, nz).bytes;
}

int mofa_iso_count(const float* grid, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace, int64_t* counts, void* stream) {
    MOFA_REQUIRE(grid && workspace && counts, "iso_count: null pointer");
    MOFA_ISO_GRID("iso_count");
    MOFA_REQUIRE(isfinite(level), "iso_count: the level must be finite (got %g)", (double)level);
    const IsoLayout l = iso_layout(nx, ny, nz);
    char* ws = (char*)workspace;
    unsigned char* eflags = (unsigned char*)(ws + l.eflags);
    unsigned char* ccounts = (unsigned char*)(ws + l.ccounts);
    long long* escan = (long long*)(ws + l.escan);
    long long* cscan = (long long*)(ws + l.cscan);
    long long* aux = (long long*)(ws + l.aux);
    long long* totals = (long long*)(ws + l.totals);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_iso_edge_flags, dim3(blocks_of(l.n_edges)), dim3(256), 0, st, grid, (long long)nx, (long long)ny, (long long)nz, level,
                       eflags);
    hipLaunchKernelGGL(k_iso_cell_counts, dim3(blocks_of(l.n_cells)), dim3(256), 0, st, grid, (long long)nx, (long long)ny, (long long)nz, level,
                       ccounts);
    int rc = check_launch("k_iso_edge_flags / k_iso_cell_counts");
    if (rc != MOFA_OK) return rc;
    if ((rc = scan_exclusive<unsigned char>(eflags, l.n_edges, escan, aux, st)) != MOFA_OK) return rc;
    if ((rc = scan_exclusive<unsigned char>(ccounts, l.n_cells, cscan, aux, st)) != MOFA_OK) return rc;
    hipLaunchKernelGGL(k_iso_totals, dim3(1), dim3(64), 0, st, (const long long*)escan, (const unsigned char*)eflags, l.n_edges,
                       (const long long*)cscan, (const unsigned char*)ccounts, l.n_cells, totals, (long long*)counts);
    return check_launch("k_iso_totals");
}

int mofa_iso_emit(const float* grid, int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], float level, void* workspace,
                  float* verts, int32_t* faces, void* stream) {
    MOFA_REQUIRE(grid && lo && step && workspace && verts && faces, "iso_emit: null pointer");
    MOFA_ISO_GRID("iso_emit");
    MOFA_REQUIRE(isfinite(level), "iso_emit: the level must be finite (got %g)", (double)level);
    for (int a = 0; a < 3; ++a)
        MOFA_REQUIRE(isfinite(lo[a]) && isfinite(step[a]) && step[a] > 0.f, "iso_emit: lo[%d] = %g, step[%d] = %g (want finite, step > 0)", a,
                     (double)lo[a], a, (double)step[a]);
    const IsoLayout l = iso_layout(nx, ny, nz);
    const char* ws = (const char*)workspace;
    const unsigned char* eflags = (const unsigned char*)(ws + l.eflags);
    const unsigned char* ccounts = (const unsigned char*)(ws + l.ccounts);
    const long long* escan = (const long long*)(ws + l.escan);
    const long long* cscan = (const long long*)(ws + l.cscan);
    const long long* totals = (const long long*)(ws + l.totals);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_iso_vertices, dim3(blocks_of(l.n_edges)), dim3(256), 0, st, grid, (long long)nx, (long long)ny, (long long)nz, level,
                       lo[0], lo[1], lo[2], step[0], step[1], step[2], eflags, escan, totals, verts);
    hipLaunchKernelGGL(k_iso_faces, dim3(blocks_of(l.n_cells)), dim3(256), 0, st, grid, (long long)nx, (long long)ny, (long long)nz, level,
                       ccounts, cscan, escan, totals, faces);
    return check_launch("k_iso_vertices / k_iso_faces");
}

int mofa_iso_edge_ids(int64_t nx, int64_t ny, int64_t nz, const void* workspace, int64_t* edge_ids, void* stream) {
    MOFA_REQUIRE(workspace && edge_ids, "iso_edge_ids: null pointer");
    MOFA_ISO_GRID("iso_edge_ids");
    const IsoLayout l = iso_layout(nx, ny, nz);
    const char* ws = (const char*)workspace;
    hipLaunchKernelGGL(k_iso_edge_ids, dim3(blocks_of(l.n_edges)), dim3(256), 0, (hipStream_t)stream, l.n_edges,
                       (const unsigned char*)(ws + l.eflags), (const long long*)(ws + l.escan), (const long long*)(ws + l.totals), edge_ids);
    return check_launch("k_iso_edge_ids");
}

}  // extern "C"

// ---- narrow-band ("sparse brick") extraction -----------------------------------------------------------------------------------------
// The fine lattice above, cut into bricks of B x B x B cells (B in {4, 8, 16}, (n - 1) % B == 0 on every axis): brick (bi,bj,bk) covers
// cells [bi B, (bi+1) B) per axis, brick index (bi * by + bj) * bz + bk, and samples the (B+1)^3 lattice points it touches (the apron is
// shared with its neighbours).  Densities are only asked for at the brick-corner lattice (seeding) and at the points of active bricks:
//
//   seed     a brick whose 8 corners are not all on one side of the level is active
//   grow     a cell of an active brick's outer layer (local index 0 or B-1 on some axis) with a triangle activates every neighbour brick it
//            touches across a face, an edge or a corner; only the bricks just evaluated are examined; repeat until nothing is added
//   own      a lattice point belongs to brick min(i / B, bx - 1) per axis, and owns the edges that leave it: every lattice edge has one
//            owner, and an edge in a triangle of an active brick's cell belongs to that brick or to a neighbour the growth activated
//   order    vertices by brick, then local owned edge (= increasing edge_id within the brick); faces by brick, local cell, tet, triangle
//
// Memory: O(1) per brick of the brick grid (flags, a scan, the density slot and the brick lists: the band workspace) plus, per ACTIVE
// brick, its (B+1)^3 densities (the caller's) and a table of 7 (B+1)^3 local vertex ranks (uint16; the mesh workspace).  Kernels:
// k_band_corner_points, k_band_seed, k_band_points, k_band_grow, k_band_round (+ k_band_compact: a round's list), k_band_sorted,
// k_band_count<B>, k_band_mesh_totals, k_band_emit<B>.
namespace mofa {
namespace {

constexpr long long kBandMaxAxis = 1ll << 24;        // (float)i is exact: the grid_coord formula holds
constexpr long long kBandMaxCorners = 1ll << 31;     // (bx+1)(by+1)(bz+1): brick ids and slots fit int32
constexpr long long kBandMaxBlocks = 1ll << 14;      // workgroups (one per brick) per launch of the per-brick kernels

struct BandGrid {
    long long nx, ny, nz;                             // lattice points per axis
    long long bx, by, bz;                             // bricks per axis
    int B;
    __host__ __device__ long long bricks() const { return bx * by * bz; }
};

// workspace words: totals[0] = bricks added by the last seed / grow (the current list), [1] = the slot of its first brick, [2] = active
enum { kTotNew = 0, kTotBase = 1, kTotActive = 2, kTotWords = 4 };

__device__ __forceinline__ void brick_coords(const BandGrid& g, long long b, long long& bi, long long& bj, long long& bk) {
    bi = b / (g.by * g.bz);
    const long long r = b - bi * (g.by * g.bz);
    bj = r / g.bz;
    bk = r - bj * g.bz;
}

// the brick-corner lattice: corner c = (ci * (by+1) + cj) * (bz+1) + ck at lattice point (ci B, cj B, ck B)
__global__ __launch_bounds__(256) void k_band_corner_points(BandGrid g, float lox, float loy, float loz, float sx, float sy, float sz,
                                                            long long first, long long n, float* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long long c = first + t, cy = g.by + 1, cz = g.bz + 1;
    const long long ci = c / (cy * cz), r = c - ci * (cy * cz), cj = r / cz, ck = r - cj * cz;
    pts[t * 3 + 0] = grid_coord(lox, sx, ci * g.B);
    pts[t * 3 + 1] = grid_coord(loy, sy, cj * g.B);
    pts[t * 3 + 2] = grid_coord(loz, sz, ck * g.B);
}

// grow[b] = the brick's corners straddle the level; active[b] = 0; the totals start over
__global__ __launch_bounds__(256) void k_band_seed(BandGrid g, const float* __restrict__ corner_sigma, float level, unsigned char* __restrict__ grow,
                                                   unsigned char* __restrict__ active, long long* __restrict__ totals) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b == 0)
        for (int w = 0; w < kTotWords; ++w) totals[w] = 0;
    if (b >= g.bricks()) return;
    long long bi, bj, bk;
    brick_coords(g, b, bi, bj, bk);
    const long long cy = g.by + 1, cz = g.bz + 1;
    unsigned in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        in |= (inside(corner_sigma[((bi + (c & 1)) * cy + bj + ((c >> 1) & 1)) * cz + bk + (c >> 2)], level) ? 1u : 0u) << c;
    grow[b] = (in != 0u && in != 0xffu) ? 1 : 0;
    active[b] = 0;
}

// the bricks flagged in `grow` become the current list: how many, the slot of the first, the running active count
__global__ void k_band_round(const unsigned char* __restrict__ grow, const long long* __restrict__ scan, long long n_bricks,
                             long long* __restrict__ totals, long long* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    const long long added = scan[n_bricks - 1] + grow[n_bricks - 1];
    totals[kTotNew] = added;
    totals[kTotBase] = totals[kTotActive];
    totals[kTotActive] += added;
    counts[0] = added, counts[1] = totals[kTotActive];
}

// list[q] = the q-th flagged brick (ascending), its densities at slot base + q; the flag moves from `grow` to `active`
__global__ __launch_bounds__(256) void k_band_compact(long long n_bricks, const long long* __restrict__ scan, const long long* __restrict__ totals,
                                                      unsigned char* __restrict__ grow, unsigned char* __restrict__ active,
                                                      int* __restrict__ list, int* __restrict__ dslot) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_bricks || !grow[b]) return;
    const long long q = scan[b];
    list[q] = (int)b;
    dslot[b] = (int)(totals[kTotBase] + q);
    active[b] = 1;
    grow[b] = 0;
}

// the (B+1)^3 lattice points of the current list's bricks: point p = q (B+1)^3 + local, local = (li (B+1) + lj) (B+1) + lk
__global__ __launch_bounds__(256) void k_band_points(BandGrid g, float lox, float loy, float loz, float sx, float sy, float sz,
                                                     const int* __restrict__ list, const long long* __restrict__ totals, long long first,
                                                     long long n, float* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long e = g.B + 1, P = e * e * e, p = first + t;
    if (t >= n || p >= totals[kTotNew] * P) return;
    const long long q = p / P, l = p - q * P, li = l / (e * e), lj = (l / e) % e, lk = l % e;
    long long bi, bj, bk;
    brick_coords(g, list[q], bi, bj, bk);
    pts[t * 3 + 0] = grid_coord(lox, sx, bi * g.B + li);
    pts[t * 3 + 1] = grid_coord(loy, sy, bj * g.B + lj);
    pts[t * 3 + 2] = grid_coord(loz, sz, bk * g.B + lk);
}

// one workgroup per brick of the current list: an outer-layer cell with a triangle (its 8 corners not all on one side) flags every
// neighbour brick it touches that is not active yet.  Concurrent stores to one flag all write 1.
__global__ __launch_bounds__(256) void k_band_grow(BandGrid g, const float* __restrict__ sigma, float level, const int* __restrict__ list,
                                                   const int* __restrict__ dslot, const long long* __restrict__ totals,
                                                   const unsigned char* __restrict__ active, unsigned char* __restrict__ grow, long long q0) {
    const long long q = q0 + blockIdx.x;
    if (q >= totals[kTotNew]) return;
    const int B = g.B, e = B + 1;
    const long long b = list[q];
    const float* s = sigma + (long long)dslot[b] * e * e * e;
    long long bi, bj, bk;
    brick_coords(g, b, bi, bj, bk);
    for (int c = threadIdx.x; c < B * B * B; c += 256) {
        const int ci = c / (B * B), cj = (c / B) % B, ck = c % B;
        const int lx = ci == 0 ? -1 : 0, hx = ci == B - 1 ? 1 : 0, ly = cj == 0 ? -1 : 0, hy = cj == B - 1 ? 1 : 0;
        const int lz = ck == 0 ? -1 : 0, hz = ck == B - 1 ? 1 : 0;
        if (lx == 0 && hx == 0 && ly == 0 && hy == 0 && lz == 0 && hz == 0) continue;       // an inner cell
        unsigned in = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            in |= (inside(s[((ci + (k & 1)) * e + cj + ((k >> 1) & 1)) * e + ck + (k >> 2)], level) ? 1u : 0u) << k;
        if (in == 0u || in == 0xffu) continue;
        for (int ox = lx; ox <= hx; ++ox)
            for (int oy = ly; oy <= hy; ++oy)
                for (int oz = lz; oz <= hz; ++oz) {
                    const long long ni = bi + ox, nj = bj + oy, nk = bk + oz;
                    if ((ox | oy | oz) == 0 || ni < 0 || nj < 0 || nk < 0 || ni >= g.bx || nj >= g.by || nk >= g.bz) continue;
                    const long long nb = (ni * g.by + nj) * g.bz + nk;
                    if (!active[nb]) grow[nb] = 1;
                }
    }
}

// list[rank] = the active bricks in ascending index (rank = the exclusive scan of the active flags), for the first n_active of them
__global__ __launch_bounds__(256) void k_band_sorted(long long n_bricks, const unsigned char* __restrict__ active,
                                                     const long long* __restrict__ rank, long long n_active, int* __restrict__ list,
                                                     int64_t* __restrict__ bricks) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_bricks || !active[b] || rank[b] >= n_active) return;
    list[rank[b]] = (int)b;
    if (bricks) bricks[rank[b]] = b;
}

// exclusive scan of one value per thread across the workgroup (256 threads); `part` is LDS
__device__ __forceinline__ long long block_exclusive_scan(long long v, long long* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const long long add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    const long long r = part[threadIdx.x] - v;
    __syncthreads();
    return r;
}

// a brick's (B+1)^3 densities into LDS
template <int B>
__device__ __forceinline__ void load_brick(const float* __restrict__ src, float* sh) {
    constexpr int P = (B + 1) * (B + 1) * (B + 1);
    for (int l = threadIdx.x; l < P; l += 256) sh[l] = src[l];
    __syncthreads();
}

// edge slot = local point * 7 + dir of a brick: owned (its lower end owned by the brick, its upper end in the brick) and crossing
template <int B>
__device__ __forceinline__ bool band_edge(const float* sh, int slot, int hx, int hy, int hz, float level, int& li, int& lj, int& lk, int& dir) {
    constexpr int e = B + 1;
    const int l = slot / 7;
    dir = slot - l * 7;
    li = l / (e * e), lj = (l / e) % e, lk = l % e;
    if (li > hx || lj > hy || lk > hz) return false;
    const int i2 = li + kDirDx[dir], j2 = lj + kDirDy[dir], k2 = lk + kDirDz[dir];
    if (i2 > B || j2 > B || k2 > B) return false;
    return inside(sh[l], level) != inside(sh[(i2 * e + j2) * e + k2], level);
}

template <int B>
__device__ __forceinline__ unsigned cell_inside(const float* sh, int c, float level) {
    constexpr int e = B + 1;
    const int ci = c / (B * B), cj = (c / B) % B, ck = c % B;
    unsigned in = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) in |= (inside(sh[((ci + (k & 1)) * e + cj + ((k >> 1) & 1)) * e + ck + (k >> 2)], level) ? 1u : 0u) << k;
    return in;
}

template <int B>
__device__ __forceinline__ int cell_triangles(unsigned in) {
    int n = 0;
    for (int t = 0; t < 6; ++t) {
        int cc[4];
        tet_corners(t, cc);
        n += tet_triangles((int)((in >> cc[0]) & 1) + (int)((in >> cc[1]) & 1) + (int)((in >> cc[2]) & 1) + (int)((in >> cc[3]) & 1));
    }
    return n;
}

// one workgroup per active brick (rank r): nv[r] = owned crossing edges, nf[r] = triangles of its B^3 cells, ranks[r][slot] = the local
// vertex number of every owned crossing edge slot (0xffff elsewhere)
template <int B>
__global__ __launch_bounds__(256) void k_band_count(BandGrid g, const float* __restrict__ sigma, float level, const int* __restrict__ list,
                                                    const int* __restrict__ dslot, const long long* __restrict__ totals, int* __restrict__ nv,
                                                    int* __restrict__ nf, unsigned short* __restrict__ ranks, long long r0) {
    constexpr int e = B + 1, P = e * e * e, E = 7 * P, S = (E + 255) / 256, C = B * B * B;
    __shared__ float sh[P];
    __shared__ long long part[256];
    const long long r = r0 + blockIdx.x;
    if (r >= totals[kTotActive]) return;
    const long long b = list[r];
    load_brick<B>(sigma + (long long)dslot[b] * P, sh);
    long long bi, bj, bk;
    brick_coords(g, b, bi, bj, bk);
    const int hx = bi == g.bx - 1 ? B : B - 1, hy = bj == g.by - 1 ? B : B - 1, hz = bk == g.bz - 1 ? B : B - 1;
    const int s0 = threadIdx.x * S, s1 = s0 + S < E ? s0 + S : E;
    int li, lj, lk, dir, n = 0;
    for (int s = s0; s < s1; ++s) n += band_edge<B>(sh, s, hx, hy, hz, level, li, lj, lk, dir);
    int v = (int)block_exclusive_scan(n, part);
    unsigned short* rk = ranks + r * E;
    for (int s = s0; s < s1; ++s) rk[s] = band_edge<B>(sh, s, hx, hy, hz, level, li, lj, lk, dir) ? (unsigned short)v++ : (unsigned short)0xffff;
    if (threadIdx.x == 255) nv[r] = v;
    int f = 0;
    for (int c = threadIdx.x; c < C; c += 256) f += cell_triangles<B>(cell_inside<B>(sh, c, level));
    const long long fe = block_exclusive_scan(f, part);
    if (threadIdx.x == 255) nf[r] = (int)(fe + f);
}

__global__ void k_band_mesh_totals(const long long* __restrict__ vscan, const int* __restrict__ nv, const long long* __restrict__ fscan,
                                   const int* __restrict__ nf, long long n, long long* __restrict__ mtotals, long long* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    const long long V = vscan[n - 1] + nv[n - 1], F = fscan[n - 1] + nf[n - 1];
    mtotals[0] = V, mtotals[1] = F;
    counts[0] = V, counts[1] = F;
}

// one workgroup per active brick (rank r): its vertices (at vbase[r] + local rank) and edge ids, and the faces of its cells in cell order
// (at fbase[r] + a workgroup scan of the per-cell counts).  A face corner on an edge of a neighbour brick Y reads Y's rank table.
template <int B>
__global__ __launch_bounds__(256) void k_band_emit(BandGrid g, float lox, float loy, float loz, float sx, float sy, float sz,
                                                   const float* __restrict__ sigma, float level, const int* __restrict__ list,
                                                   const int* __restrict__ dslot, const long long* __restrict__ rank_of,
                                                   const unsigned char* __restrict__ active, const long long* __restrict__ totals,
                                                   const long long* __restrict__ mtotals, const long long* __restrict__ vbase,
                                                   const long long* __restrict__ fbase, const unsigned short* __restrict__ ranks,
                                                   float* __restrict__ verts, int64_t* __restrict__ edge_ids, int* __restrict__ faces,
                                                   long long r0) {
    constexpr int e = B + 1, P = e * e * e, E = 7 * P, C = B * B * B, SC = (C + 255) / 256;
    __shared__ float sh[P];
    __shared__ long long part[256];
    const long long r = r0 + blockIdx.x;
    if (r >= totals[kTotActive] || mtotals[0] > kIsoMaxOut || mtotals[1] > kIsoMaxOut) return;   // (refused: the host saw the counts)
    const long long b = list[r];
    load_brick<B>(sigma + (long long)dslot[b] * P, sh);
    long long bi, bj, bk;
    brick_coords(g, b, bi, bj, bk);
    const int hx = bi == g.bx - 1 ? B : B - 1, hy = bj == g.by - 1 ? B : B - 1, hz = bk == g.bz - 1 ? B : B - 1;
    const unsigned short* rk = ranks + r * E;
    for (int s = threadIdx.x; s < E; s += 256) {
        int li, lj, lk, dir;
        if (!band_edge<B>(sh, s, hx, hy, hz, level, li, lj, lk, dir)) continue;
        const long long v = vbase[r] + rk[s];
        const long long i = bi * B + li, j = bj * B + lj, k = bk * B + lk;
        const long long i2 = i + kDirDx[dir], j2 = j + kDirDy[dir], k2 = k + kDirDz[dir];
        const float sa = sh[(li * e + lj) * e + lk], sb = sh[((li + kDirDx[dir]) * e + lj + kDirDy[dir]) * e + lk + kDirDz[dir]];
        const float t = __fdiv_rn(__fsub_rn(level, sa), __fsub_rn(sb, sa));
        const float pa[3] = {grid_coord(lox, sx, i), grid_coord(loy, sy, j), grid_coord(loz, sz, k)};
        const float pb[3] = {grid_coord(lox, sx, i2), grid_coord(loy, sy, j2), grid_coord(loz, sz, k2)};
#pragma unroll
        for (int a = 0; a < 3; ++a) verts[v * 3 + a] = __fadd_rn(pa[a], __fmul_rn(t, __fsub_rn(pb[a], pa[a])));
        edge_ids[v] = 7 * ((i * g.ny + j) * g.nz + k) + dir;
    }
    // faces: thread t takes the cells [t SC, (t+1) SC) so that a workgroup scan of its counts orders them by cell
    const int c0 = threadIdx.x * SC, c1 = c0 + SC < C ? c0 + SC : C;
    int n = 0;
    for (int c = c0; c < c1; ++c) n += cell_triangles<B>(cell_inside<B>(sh, c, level));
    long long f = fbase[r] + block_exclusive_scan(n, part);
    // the vertex id of the edge (lower end at local point l of this brick, direction dir): its owner brick per axis is this one, or the
    // next one when the point lies on the brick's upper face and the brick is not the last on that axis
    auto vid = [&](int li, int lj, int lk, int dir) -> long long {
        const int ox = li == B && bi < g.bx - 1, oy = lj == B && bj < g.by - 1, oz = lk == B && bk < g.bz - 1;
        long long ry = r;
        if (ox | oy | oz) {
            const long long y = ((bi + ox) * g.by + bj + oy) * g.bz + bk + oz;
            if (!active[y]) return -1;                                          // (unreachable: the growth activated it)
            ry = rank_of[y];
        }
        const int slot = (((li - ox * B) * e + lj - oy * B) * e + lk - oz * B) * 7 + dir;
        return vbase[ry] + ranks[ry * E + slot];
    };
    for (int c = c0; c < c1; ++c) {
        const unsigned in = cell_inside<B>(sh, c, level);
        if (in == 0u || in == 0xffu) continue;
        const int ci = c / (B * B), cj = (c / B) % B, ck = c % B;
        for (int t = 0; t < 6; ++t) {
            long long tri[2][3];
            const int n_tri = tet_tris(in, t, [&](int lo, int, int dir) { return vid(ci + (lo & 1), cj + ((lo >> 1) & 1), ck + (lo >> 2), dir); },
                                       tri);
            for (int s = 0; s < n_tri; ++s, ++f)
                for (int a = 0; a < 3; ++a) faces[f * 3 + a] = (int)tri[s][a];
        }
    }
}

// a grid the band extraction takes (checked without overflow): B in {4, 8, 16}, (n - 1) % B == 0 and 2 <= n < 2^24 on every axis, and
// fewer than 2^31 brick corners
int band_grid_check(long long nx, long long ny, long long nz, int B, const char* what) {
    MOFA_REQUIRE(B == 4 || B == 8 || B == 16, "%s: brick size %d (want 4, 8 or 16)", what, B);
    MOFA_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && nx < kBandMaxAxis && ny < kBandMaxAxis && nz < kBandMaxAxis,
                 "%s: grid %lld x %lld x %lld is too large or too small (2 <= n < 2^24 per axis)", what, nx, ny, nz);
    MOFA_REQUIRE((nx - 1) % B == 0 && (ny - 1) % B == 0 && (nz - 1) % B == 0,
                 "%s: grid %lld x %lld x %lld does not split into bricks of %d cells ((n - 1) %% B must be 0)", what, nx, ny, nz, B);
    const long long cx = (nx - 1) / B + 1, cy = (ny - 1) / B + 1, cz = (nz - 1) / B + 1;
    MOFA_REQUIRE(cx * cy < kBandMaxCorners && cx * cy * cz < kBandMaxCorners,
                 "%s: grid %lld x %lld x %lld is too large (%lld x %lld x %lld brick corners, want fewer than 2^31)", what, nx, ny, nz, cx, cy, cz);
    return MOFA_OK;
}

// workgroups of the launch that starts at brick r0 of n
inline unsigned brick_blocks(long long n, long long r0) { return (unsigned)(n - r0 < kBandMaxBlocks ? n - r0 : kBandMaxBlocks); }

BandGrid band_grid(long long nx, long long ny, long long nz, int B) {
    return BandGrid{nx, ny, nz, (nx - 1) / B, (ny - 1) / B, (nz - 1) / B, B};
}

int band_geometry_check(const float lo[3], const float step[3], const char* what) {
    for (int a = 0; a < 3; ++a)
        MOFA_REQUIRE(isfinite(lo[a]) && isfinite(step[a]) && step[a] > 0.f, "%s: lo[%d] = %g, step[%d] = %g (want finite, step > 0)", what, a,
                     (double)lo[a], a, (double)step[a]);
    return MOFA_OK;
}

// *dst = *src (one device int64) once the work queued on `st` has run: a host synchronisation
int band_read_total(const long long* src, long long* dst, hipStream_t st, const char* what) {
    if (hipMemcpyAsync(dst, src, sizeof(long long), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        set_error("%s: reading a count back from the device failed", what);
        return MOFA_EHIP;
    }
    return MOFA_OK;
}

// the caller's n_active must be the workspace's: the mesh workspace, the brick list and the launches are sized by it
int band_active_check(const long long* totals, long long n_active, hipStream_t st, const char* what) {
    long long active = 0;
    const int rc = band_read_total(totals + kTotActive, &active, st, what);
    if (rc != MOFA_OK) return rc;
    MOFA_REQUIRE(active == n_active, "%s: n_active = %lld, but the workspace holds %lld active bricks", what, n_active, active);
    return MOFA_OK;
}

// the band workspace: O(1) per brick of the brick grid
struct BandLayout {
    size_t active, grow, scan, aux, dslot, list, totals, bytes;
};
BandLayout band_layout(const BandGrid& g) {
    const long long nb = g.bricks();
    BandLayout l{};
    size_t o = 0;
    l.active = o, o = align_up(o + (size_t)nb);
    l.grow = o, o = align_up(o + (size_t)nb);
    l.scan = o, o = align_up(o + (size_t)nb * 8);
    l.aux = o, o = align_up(o + (size_t)scan_aux(nb) * 8);
    l.dslot = o, o = align_up(o + (size_t)nb * 4);
    l.list = o, o = align_up(o + (size_t)nb * 4);
    l.totals = o, o = align_up(o + kTotWords * 8);
    l.bytes = o;
    return l;
}

// the mesh workspace: per active brick its counts, their scans and its rank table
struct BandMeshLayout {
    size_t nv, nf, vbase, fbase, aux, totals, ranks, bytes;
};
BandMeshLayout band_mesh_layout(int B, long long n_active) {
    const long long E = 7ll * (B + 1) * (B + 1) * (B + 1);
    BandMeshLayout l{};
    size_t o = 0;
    l.nv = o, o = align_up(o + (size_t)n_active * 4);
    l.nf = o, o = align_up(o + (size_t)n_active * 4);
    l.vbase = o, o = align_up(o + (size_t)n_active * 8);
    l.fbase = o, o = align_up(o + (size_t)n_active * 8);
    l.aux = o, o = align_up(o + (size_t)scan_aux(n_active) * 8);
    l.totals = o, o = align_up(o + 2 * 8);
    l.ranks = o, o = align_up(o + (size_t)(n_active * E) * 2);
    l.bytes = o;
    return l;
}

struct BandWs {
    unsigned char *active, *grow;
    long long *scan, *aux, *totals;
    int *dslot, *list;
};
BandWs band_ws(const BandGrid& g, void* workspace) {
    const BandLayout l = band_layout(g);
    char* ws = (char*)workspace;
    return BandWs{(unsigned char*)(ws + l.active), (unsigned char*)(ws + l.grow), (long long*)(ws + l.scan), (long long*)(ws + l.aux),
                  (long long*)(ws + l.totals), (int*)(ws + l.dslot), (int*)(ws + l.list)};
}

// the bricks flagged in w.grow become the current list (scan, counts, compaction)
int band_round(const BandGrid& g, const BandWs& w, int64_t* counts, hipStream_t st) {
    const long long nb = g.bricks();
    int rc = scan_exclusive<unsigned char>(w.grow, nb, w.scan, w.aux, st);
    if (rc != MOFA_OK) return rc;
    hipLaunchKernelGGL(k_band_round, dim3(1), dim3(64), 0, st, (const unsigned char*)w.grow, (const long long*)w.scan, nb, w.totals,
                       (long long*)counts);
    hipLaunchKernelGGL(k_band_compact, dim3(blocks_of(nb)), dim3(256), 0, st, nb, (const long long*)w.scan, (const long long*)w.totals, w.grow,
                       w.active, w.list, w.dslot);
    return check_launch("k_band_round / k_band_compact");
}

template <int B>
void launch_band_count(const BandGrid& g, const float* sigma, float level, const BandWs& w, long long n, int* nv, int* nf,
                       unsigned short* ranks, hipStream_t st) {
    for (long long r0 = 0; r0 < n; r0 += kBandMaxBlocks)
        hipLaunchKernelGGL(k_band_count<B>, dim3(brick_blocks(n, r0)), dim3(256), 0, st, g, sigma, level, (const int*)w.list,
                           (const int*)w.dslot, (const long long*)w.totals, nv, nf, ranks, r0);
}

template <int B>
void launch_band_emit(const BandGrid& g, const float* lo, const float* step, const float* sigma, float level, const BandWs& w, long long n,
                      const long long* mtotals, const long long* vbase, const long long* fbase, const unsigned short* ranks, float* verts,
                      int64_t* edge_ids, int* faces, hipStream_t st) {
    for (long long r0 = 0; r0 < n; r0 += kBandMaxBlocks)
        hipLaunchKernelGGL(k_band_emit<B>, dim3(brick_blocks(n, r0)), dim3(256), 0, st, g, lo[0], lo[1], lo[2], step[0], step[1], step[2], sigma,
                           level, (const int*)w.list, (const int*)w.dslot, (const long long*)w.scan, (const unsigned char*)w.active,
                           (const long long*)w.totals, mtotals, vbase, fbase, ranks, verts, edge_ids, faces, r0);
}

}  // namespace
}  // namespace mofa

#define MOFA_BAND_GRID(what)                                         \
    do {                                                             \
        const int rc_ = band_grid_check(nx, ny, nz, brick, what);    \
        if (rc_ != MOFA_OK) return rc_;                              \
    } while (0)

extern "C" {

size_t mofa_band_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, int32_t brick) {
    if (band_grid_check(nx, ny, nz, brick, "band_workspace_bytes") != MOFA_OK) return 0;
    return band_layout(band_grid(nx, ny, nz, brick)).bytes;
}

size_t mofa_band_mesh_bytes(int32_t brick, int64_t n_active) {
    if ((brick != 4 && brick != 8 && brick != 16) || n_active < 1 || n_active >= kBandMaxCorners) return 0;
    return band_mesh_layout(brick, n_active).bytes;
}

int mofa_band_corner_points(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float lo[3], const float step[3], int64_t first, int64_t n,
                            float* pts, void* stream) {
    MOFA_REQUIRE(lo && step && pts, "band_corner_points: null pointer");
    MOFA_BAND_GRID("band_corner_points");
    const int rc = band_geometry_check(lo, step, "band_corner_points");
    if (rc != MOFA_OK) return rc;
    const BandGrid g = band_grid(nx, ny, nz, brick);
    const long long n_corners = (g.bx + 1) * (g.by + 1) * (g.bz + 1);
    MOFA_REQUIRE(first >= 0 && n > 0 && first + n <= n_corners, "band_corner_points: corners [%lld, %lld) of %lld", (long long)first,
                 (long long)(first + n), n_corners);
    hipLaunchKernelGGL(k_band_corner_points, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, g, lo[0], lo[1], lo[2], step[0], step[1],
                       step[2], (long long)first, (long long)n, pts);
    return check_launch("k_band_corner_points");
}

int mofa_band_seed(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float* corner_sigma, float level, void* workspace, int64_t* counts,
                   void* stream) {
    MOFA_REQUIRE(corner_sigma && workspace && counts, "band_seed: null pointer");
    MOFA_BAND_GRID("band_seed");
    MOFA_REQUIRE(isfinite(level), "band_seed: the level must be finite (got %g)", (double)level);
    const BandGrid g = band_grid(nx, ny, nz, brick);
    const BandWs w = band_ws(g, workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_band_seed, dim3(blocks_of(g.bricks())), dim3(256), 0, st, g, corner_sigma, level, w.grow, w.active, w.totals);
    const int rc = check_launch("k_band_seed");
    if (rc != MOFA_OK) return rc;
    return band_round(g, w, counts, st);
}

int mofa_band_points(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float lo[3], const float step[3], const void* workspace,
                     int64_t n_new, int64_t first, int64_t n, float* pts, void* stream) {
    MOFA_REQUIRE(lo && step && workspace && pts, "band_points: null pointer");
    MOFA_BAND_GRID("band_points");
    const int rc = band_geometry_check(lo, step, "band_points");
    if (rc != MOFA_OK) return rc;
    const BandGrid g = band_grid(nx, ny, nz, brick);
    const long long P = (long long)(brick + 1) * (brick + 1) * (brick + 1);
    MOFA_REQUIRE(n_new >= 1 && n_new <= g.bricks() && first >= 0 && n > 0 && first + n <= n_new * P,
                 "band_points: points [%lld, %lld) of %lld bricks x %lld", (long long)first, (long long)(first + n), (long long)n_new, P);
    const BandWs w = band_ws(g, (void*)workspace);
    hipLaunchKernelGGL(k_band_points, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, g, lo[0], lo[1], lo[2], step[0], step[1], step[2],
                       (const int*)w.list, (const long long*)w.totals, (long long)first, (long long)n, pts);
    return check_launch("k_band_points");
}

int mofa_band_grow(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float* sigma, float level, void* workspace, int64_t n_new,
                   int64_t* counts, void* stream) {
    MOFA_REQUIRE(sigma && workspace && counts, "band_grow: null pointer");
    MOFA_BAND_GRID("band_grow");
    MOFA_REQUIRE(isfinite(level), "band_grow: the level must be finite (got %g)", (double)level);
    const BandGrid g = band_grid(nx, ny, nz, brick);
    MOFA_REQUIRE(n_new >= 1 && n_new <= g.bricks(), "band_grow: %lld bricks just evaluated (want 1 .. %lld)", (long long)n_new, g.bricks());
    const BandWs w = band_ws(g, workspace);
    hipStream_t st = (hipStream_t)stream;
    for (long long q0 = 0; q0 < n_new; q0 += kBandMaxBlocks)
        hipLaunchKernelGGL(k_band_grow, dim3(brick_blocks(n_new, q0)), dim3(256), 0, st, g, sigma, level, (const int*)w.list,
                           (const int*)w.dslot, (const long long*)w.totals, (const unsigned char*)w.active, w.grow, q0);
    const int rc = check_launch("k_band_grow");
    if (rc != MOFA_OK) return rc;
    return band_round(g, w, counts, st);
}

int mofa_band_count(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float* sigma, float level, void* workspace, int64_t n_active,
                    void* mesh_workspace, int64_t* counts, int64_t* bricks, void* stream) {
    MOFA_REQUIRE(sigma && workspace && mesh_workspace && counts, "band_count: null pointer");
    MOFA_BAND_GRID("band_count");
    MOFA_REQUIRE(isfinite(level), "band_count: the level must be finite (got %g)", (double)level);
    const BandGrid g = band_grid(nx, ny, nz, brick);
    MOFA_REQUIRE(n_active >= 1 && n_active <= g.bricks(), "band_count: %lld active bricks (want 1 .. %lld)", (long long)n_active, g.bricks());
    const BandWs w = band_ws(g, workspace);
    const BandMeshLayout l = band_mesh_layout(brick, n_active);
    char* mws = (char*)mesh_workspace;
    int* nv = (int*)(mws + l.nv);
    int* nf = (int*)(mws + l.nf);
    long long* vbase = (long long*)(mws + l.vbase);
    long long* fbase = (long long*)(mws + l.fbase);
    long long* aux = (long long*)(mws + l.aux);
    long long* mtotals = (long long*)(mws + l.totals);
    unsigned short* ranks = (unsigned short*)(mws + l.ranks);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = g.bricks();
    int rc = band_active_check(w.totals, n_active, st, "band_count");
    if (rc != MOFA_OK) return rc;
    if ((rc = scan_exclusive<unsigned char>(w.active, nb, w.scan, w.aux, st)) != MOFA_OK) return rc;   // w.scan: brick -> rank from here on
    hipLaunchKernelGGL(k_band_sorted, dim3(blocks_of(nb)), dim3(256), 0, st, nb, (const unsigned char*)w.active, (const long long*)w.scan,
                       (long long)n_active, w.list, bricks);
    if (brick == 4) launch_band_count<4>(g, sigma, level, w, n_active, nv, nf, ranks, st);
    else if (brick == 8) launch_band_count<8>(g, sigma, level, w, n_active, nv, nf, ranks, st);
    else launch_band_count<16>(g, sigma, level, w, n_active, nv, nf, ranks, st);
    if ((rc = check_launch("k_band_sorted / k_band_count")) != MOFA_OK) return rc;
    if ((rc = scan_exclusive<int>(nv, n_active, vbase, aux, st)) != MOFA_OK) return rc;
    if ((rc = scan_exclusive<int>(nf, n_active, fbase, aux, st)) != MOFA_OK) return rc;
    hipLaunchKernelGGL(k_band_mesh_totals, dim3(1), dim3(64), 0, st, (const long long*)vbase, (const int*)nv, (const long long*)fbase,
                       (const int*)nf, (long long)n_active, mtotals, (long long*)counts);
    return check_launch("k_band_mesh_totals");
}

int mofa_band_emit(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float lo[3], const float step[3], const float* sigma, float level,
                   const void* workspace, int64_t n_active, const void* mesh_workspace, float* verts, int64_t* edge_ids, int32_t* faces,
                   void* stream) {
    MOFA_REQUIRE(lo && step && sigma && workspace && mesh_workspace && verts && edge_ids && faces, "band_emit: null pointer");
    MOFA_BAND_GRID("band_emit");
    MOFA_REQUIRE(isfinite(level), "band_emit: the level must be finite (got %g)", (double)level);
    int rc = band_geometry_check(lo, step, "band_emit");
    if (rc != MOFA_OK) return rc;
    const BandGrid g = band_grid(nx, ny, nz, brick);
    MOFA_REQUIRE(n_active >= 1 && n_active <= g.bricks(), "band_emit: %lld active bricks (want 1 .. %lld)", (long long)n_active, g.bricks());
    const BandWs w = band_ws(g, (void*)workspace);
    const BandMeshLayout l = band_mesh_layout(brick, n_active);
    const char* mws = (const char*)mesh_workspace;
    const long long* vbase = (const long long*)(mws + l.vbase);
    const long long* fbase = (const long long*)(mws + l.fbase);
    const long long* mtotals = (const long long*)(mws + l.totals);
    const unsigned short* ranks = (const unsigned short*)(mws + l.ranks);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = band_active_check(w.totals, n_active, st, "band_emit")) != MOFA_OK) return rc;
    long long V = 0, F = 0;
    if ((rc = band_read_total(mtotals, &V, st, "band_emit")) != MOFA_OK || (rc = band_read_total(mtotals + 1, &F, st, "band_emit")) != MOFA_OK)
        return rc;
    MOFA_REQUIRE(V <= kIsoMaxOut && F <= kIsoMaxOut, "band_emit: %lld vertices / %lld faces exceed the int32 face indices (2^31 - 1)", V, F);
    if (brick == 4) launch_band_emit<4>(g, lo, step, sigma, level, w, n_active, mtotals, vbase, fbase, ranks, verts, edge_ids, faces, st);
    else if (brick == 8) launch_band_emit<8>(g, lo, step, sigma, level, w, n_active, mtotals, vbase, fbase, ranks, verts, edge_ids, faces, st);
    else launch_band_emit<16>(g, lo, step, sigma, level, w, n_active, mtotals, vbase, fbase, ranks, verts, edge_ids, faces, st);
    return check_launch("k_band_emit");
}

}  // extern "C"
