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
// Kernels: k_iso_edge_flags, k_iso_cell_counts (+ the scans and k_iso_totals: mofa_iso_count), k_iso_vertices, k_iso_faces (mofa_iso_emit).
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr int kScanItems = 8;                       // elements per thread of one scan tile
constexpr int kScanTile = 256 * kScanItems;         // elements per workgroup
constexpr long long kIsoMaxEdges = 1ll << 31;       // 7 nx ny nz must stay below this
constexpr long long kIsoMaxOut = 2147483647ll;      // V and F must fit int32 face indices

__device__ __forceinline__ float grid_coord(float lo, float step, long long i) { return __fadd_rn(lo, __fmul_rn((float)i, step)); }

__device__ __forceinline__ bool inside(float s, float level) { return s >= level; }     // (false for NaN)

// offset (dx + 2 dy + 4 dz) of a tet edge -> lattice direction 0..6 (+x, +y, +z, +x+y, +x+z, +y+z, +x+y+z)
__device__ __constant__ int kDirOfOffset[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
__device__ __constant__ int kDirDx[7] = {1, 0, 0, 1, 1, 0, 1};
__device__ __constant__ int kDirDy[7] = {0, 1, 0, 1, 0, 1, 1};
__device__ __constant__ int kDirDz[7] = {0, 0, 1, 0, 1, 1, 1};
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
        int cc[4];
        tet_corners(t, cc);
        int ins[4], n_in = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) ins[u] = (int)((in >> cc[u]) & 1), n_in += ins[u];
        if (n_in == 0 || n_in == 4) continue;
        // vertex id of the tet edge between corners u and w (the corners grow componentwise, so the lower one is min(u, w))
        auto vid = [&](int u, int w) -> int {
            const int lo = u < w ? u : w, hi = u < w ? w : u;
            return (int)escan[7 * idx[cc[lo]] + kDirOfOffset[cc[hi] ^ cc[lo]]];
        };
        int tri[2][3];
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
            const int pu = vid(p, u), pw = vid(p, w), qw = vid(q, w), qu = vid(q, u);
            tri[0][0] = pu, tri[0][1] = pw, tri[0][2] = qw;
            tri[1][0] = pu, tri[1][1] = qw, tri[1][2] = qu;
            n_tri = 2;
        }
        for (int s = 0; s < n_tri; ++s, ++f) {
            const bool flip = kPermSign[t] < 0;                // a negatively oriented tet mirrors every normal
            faces[f * 3 + 0] = tri[s][0];
            faces[f * 3 + 1] = flip ? tri[s][2] : tri[s][1];
            faces[f * 3 + 2] = flip ? tri[s][1] : tri[s][2];
        }
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

}  // extern "C"
