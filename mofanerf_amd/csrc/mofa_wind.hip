// Mesh winding numbers for the geometry export (gfx950): the signed count of the faces of a closed triangle mesh that the ray
// p + t e_a, t > 0 crosses, for many query points, through a 2-D grid of face lists over the plane across the ray.  mesh.py drives the
// passes (mesh.winding_number, mesh.signed_distance, mesh.surface_distance(signed=True), mesh.inside_grid); nothing here waits on another
// thread, no float or double atomic exists (the only atomics are the integer counters), and every kernel checks the indices it
// dereferences: a bad one is skipped, never a fault.
//
// With u = (a + 1) % 3, v = (a + 2) % 3 ((u, v, a) right-handed), all coordinates the fp32 ones widened to fp64 and every difference and
// product rounded separately, face (X0, X1, X2) and query p:
//   class     right_k = X_k.u > p.u;  all three equal: the face is not crossed
//   edges     X_k -> X_k+1 straddles when right_k != right_k+1;  L = its non-right, R = its right endpoint (the same two points in the
//             same roles for both faces of the edge, so both compute the same bits):
//               p.v >= max(L.v, R.v): not above;   p.v < min(L.v, R.v): above;
//               otherwise E = (R.u - L.u) (p.v - L.v) - (R.v - L.v) (p.u - L.u), above = E < 0
//             an edge that is above adds right_k ? +1 : -1 to w;  two edges straddle, so w is -1, 0 or +1
//   height    only when w != 0:   p.a < min X_k.a: hit;   p.a >= max X_k.a: no hit;   otherwise ab = X1 - X0, ac = X2 - X0, d = p - X0,
//             n = (ab.y ac.z - ab.z ac.y, ab.z ac.x - ab.x ac.z, ab.x ac.y - ab.y ac.x), s = (n.x d.x + n.y d.y) + n.z d.z,
//             hit = w > 0 ? s < 0 : s > 0
//   sum       a hit adds w to the winding number and 1 to the crossings
// A face can only count where min u <= p.u < max u and min v <= p.v < max v: the faces listed in the cell of (p.u, p.v) are all that
// can, whatever the resolution of the grid.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kWindMaxIndex = (1ll << 31) - 1;     // N, V, F, the pair count and the cell count: int32 indices

struct WindGrid {
    double origin[2], cell[2];
    int n[2];
};

__device__ __forceinline__ bool wind_in_range(int v, int V) { return (unsigned)v < (unsigned)V; }

__device__ __forceinline__ int wind_cell(double x, double origin, double cell, int n) {
    const double t = floor((x - origin) / cell);
    return t >= 0.0 ? (t < (double)n ? (int)t : n - 1) : 0;          // (NaN: 0)
}

__device__ __forceinline__ void wind_load(const float* __restrict__ verts, int i, double (&p)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (double)verts[(long long)i * 3 + c];
}

__device__ __forceinline__ double wind_min3(double a, double b, double c) {
    const double m = a < b ? a : b;
    return c < m ? c : m;
}

__device__ __forceinline__ double wind_max3(double a, double b, double c) {
    const double m = a > b ? a : b;
    return c > m ? c : m;
}

// what the edge a -> b (classes ra, rb) adds to w
template <int U, int V>
__device__ __forceinline__ int wind_edge(const double (&p)[3], const double (&a)[3], const double (&b)[3], bool ra, bool rb) {
    if (ra == rb) return 0;
    const double lu = ra ? b[U] : a[U], lv = ra ? b[V] : a[V], ru = ra ? a[U] : b[U], rv = ra ? a[V] : b[V];
    bool above;
    if (p[V] >= (lv > rv ? lv : rv)) {
        above = false;
    } else if (p[V] < (lv < rv ? lv : rv)) {
        above = true;
    } else {
        const double e = (ru - lu) * (p[V] - lv) - (rv - lv) * (p[U] - lu);
        above = e < 0.0;
    }
    return above ? (ra ? 1 : -1) : 0;
}

// what the face (x0, x1, x2) adds to the winding number of p along axis A: -1, 0 or +1
template <int A>
__device__ __forceinline__ int wind_face(const double (&p)[3], const double (&x0)[3], const double (&x1)[3], const double (&x2)[3]) {
    constexpr int U = (A + 1) % 3, V = (A + 2) % 3;
    const bool r0 = x0[U] > p[U], r1 = x1[U] > p[U], r2 = x2[U] > p[U];
    if (r0 == r1 && r1 == r2) return 0;
    const int w = wind_edge<U, V>(p, x0, x1, r0, r1) + wind_edge<U, V>(p, x1, x2, r1, r2) + wind_edge<U, V>(p, x2, x0, r2, r0);
    if (w == 0) return 0;
    bool hit;
    if (p[A] < wind_min3(x0[A], x1[A], x2[A])) {
        hit = true;
    } else if (p[A] >= wind_max3(x0[A], x1[A], x2[A])) {
        hit = false;
    } else {
        const double ab[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, ac[3] = {x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2]};
        const double d[3] = {p[0] - x0[0], p[1] - x0[1], p[2] - x0[2]};
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double s = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
        hit = w > 0 ? s < 0.0 : s > 0.0;
    }
    return hit ? w : 0;
}

// sums `v` over the wavefront (every lane of it must call) and adds the total to counts[slot]: one integer atomic per wavefront
__device__ __forceinline__ void wind_wave_add(int64_t* counts, int slot, unsigned long long v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w);
    if (__lane_id() == 0 && v) atomicAdd((unsigned long long*)(counts + slot), v);
}

// the index box of a face in the (u, v) grid, false for a face that enters no cell (a bad index, no extent in u or in v)
template <int A>
__device__ __forceinline__ bool wind_face_box(const float* __restrict__ verts, const int* __restrict__ faces, long long f, int V, const WindGrid& g,
                                              int (&lo)[2], int (&hi)[2], bool& flat) {
    constexpr int UV[2] = {(A + 1) % 3, (A + 2) % 3};
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    flat = false;
    if (!wind_in_range(i0, V) || !wind_in_range(i1, V) || !wind_in_range(i2, V)) return false;
    double a[3], b[3], c[3];
    wind_load(verts, i0, a), wind_load(verts, i1, b), wind_load(verts, i2, c);
    double mn[2], mx[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) mn[k] = wind_min3(a[UV[k]], b[UV[k]], c[UV[k]]), mx[k] = wind_max3(a[UV[k]], b[UV[k]], c[UV[k]]);
    if (mn[0] == mx[0] || mn[1] == mx[1]) {
        flat = true;
        return false;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) lo[k] = wind_cell(mn[k], g.origin[k], g.cell[k], g.n[k]), hi[k] = wind_cell(mx[k], g.origin[k], g.cell[k], g.n[k]);
    return lo[0] <= hi[0] && lo[1] <= hi[1];                      // (always, for finite vertices: the cell index is monotone)
}

template <int A>
__global__ __launch_bounds__(256) void k_wind_bin_count(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V, WindGrid g,
                                                        int64_t* __restrict__ n_cells, int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool flat = false;
    if (f < F) {
        int lo[2], hi[2];
        long long n = 0;
        if (wind_face_box<A>(verts, faces, f, V, g, lo, hi, flat)) n = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1);
        n_cells[f] = n;
    }
    const unsigned long long b = __ballot(flat);
    if (flat && (int)__lane_id() == __ffsll(b) - 1) atomicAdd((unsigned long long*)(counts + MOFA_WIND_FLAT), (unsigned long long)__popcll(b));
}

template <int A>
__global__ __launch_bounds__(256) void k_wind_bin_emit(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V, WindGrid g,
                                                       const int64_t* __restrict__ offsets, long long P, int* __restrict__ pair_cell,
                                                       int* __restrict__ pair_face) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int lo[2], hi[2];
    bool flat;
    if (!wind_face_box<A>(verts, faces, f, V, g, lo, hi, flat)) return;
    long long o = offsets[f];
    for (int iu = lo[0]; iu <= hi[0]; ++iu)
        for (int iv = lo[1]; iv <= hi[1]; ++iv, ++o) {
            if (o < 0 || o >= P) return;                                         // (offsets that do not belong to this mesh and grid)
            pair_cell[o] = iu * g.n[1] + iv;
            pair_face[o] = (int)f;
        }
}

template <int A>
__global__ __launch_bounds__(256) void k_wind_query(const float* __restrict__ points, long long N, const int64_t* __restrict__ order,
                                                    const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                    const int* __restrict__ cell_start, const int* __restrict__ pair_face, int P, WindGrid g,
                                                    int* __restrict__ winding, int* __restrict__ crossings, int64_t* __restrict__ counts) {
    constexpr int U = (A + 1) % 3, W = (A + 2) % 3;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long q = -1;
    if (i < N) {
        q = order ? order[i] : i;
        if (q < 0 || q >= N) q = -1;
    }
    unsigned long long tests = 0;
    int column = 0;
    bool non_finite = false;
    if (q >= 0) {
        const float pf[3] = {points[q * 3 + 0], points[q * 3 + 1], points[q * 3 + 2]};
        const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        non_finite = !(isfinite(pf[0]) && isfinite(pf[1]) && isfinite(pf[2]));
        int wn = 0, cr = 0;
        if (!non_finite && P > 0) {
            const int col = wind_cell(p[U], g.origin[0], g.cell[0], g.n[0]) * g.n[1] + wind_cell(p[W], g.origin[1], g.cell[1], g.n[1]);
            int j0 = cell_start[col], j1 = cell_start[col + 1];
            j0 = j0 < 0 ? 0 : j0, j1 = j1 > P ? P : j1;
            for (int j = j0; j < j1; ++j) {
                const int f = pair_face[j];
                if (!wind_in_range(f, F)) continue;
                const int i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
                if (!wind_in_range(i0, V) || !wind_in_range(i1, V) || !wind_in_range(i2, V)) continue;
                double x0[3], x1[3], x2[3];
                wind_load(verts, i0, x0), wind_load(verts, i1, x1), wind_load(verts, i2, x2);
                ++tests;
                const int w = wind_face<A>(p, x0, x1, x2);
                wn += w, cr += w != 0;
            }
            column = j1 > j0 ? j1 - j0 : 0;
        }
        winding[q] = wn, crossings[q] = cr;
    }
    wind_wave_add(counts, MOFA_WIND_NON_FINITE, non_finite ? 1ull : 0ull);
    wind_wave_add(counts, MOFA_WIND_TESTS, tests);
    int m = column;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) m = max(m, __shfl_xor(m, w));
    if (__lane_id() == 0 && m > 0) atomicMax((unsigned long long*)(counts + MOFA_WIND_MAX_COLUMN), (unsigned long long)m);
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

bool wind_grid(const double* origin, const double* cell, const int32_t* n, WindGrid& g) {
    for (int a = 0; a < 2; ++a) {
        g.origin[a] = origin[a], g.cell[a] = cell[a], g.n[a] = n[a];
        if (!isfinite(origin[a]) || !isfinite(cell[a]) || !(cell[a] > 0.0)) return false;
        if (n[a] < 1 || n[a] > MOFA_WIND_MAX_GRID) return false;
    }
    return true;                                                 // (at most 4096^2 cells: they fit an int32)
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_WIND_COUNT(what, name, n) \
    MOFA_REQUIRE((n) >= 1 && (n) <= kWindMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))
#define MOFA_WIND_GRID(what)                                                                                           \
    MOFA_REQUIRE(axis >= 0 && axis <= 2, what ": axis = %d (want 0, 1 or 2)", (int)axis);                              \
    MOFA_REQUIRE(wind_grid(origin, cell, n, g), what ": origin / cell must be finite, cell > 0, 1 <= n <= 4096 per axis")
#define MOFA_WIND_LAUNCH(kernel, count, ...)                                                                           \
    switch (axis) {                                                                                                    \
        case 0: hipLaunchKernelGGL(kernel<0>, dim3(blocks_of(count)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 1: hipLaunchKernelGGL(kernel<1>, dim3(blocks_of(count)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL(kernel<2>, dim3(blocks_of(count)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }

extern "C" {

int mofa_wind_bin_count(const float* verts, const int32_t* faces, int64_t F, int64_t V, int32_t axis, const double origin[2], const double cell[2],
                        const int32_t n[2], int64_t* n_cells, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts && faces && origin && cell && n && n_cells && counts, "wind_bin_count: null pointer");
    MOFA_WIND_COUNT("wind_bin_count", "F", F);
    MOFA_WIND_COUNT("wind_bin_count", "V", V);
    WindGrid g;
    MOFA_WIND_GRID("wind_bin_count");
    MOFA_WIND_LAUNCH(k_wind_bin_count, F, verts, faces, (long long)F, (int)V, g, n_cells, counts);
    return check_launch("k_wind_bin_count");
}

int mofa_wind_bin_emit(const float* verts, const int32_t* faces, int64_t F, int64_t V, int32_t axis, const double origin[2], const double cell[2],
                       const int32_t n[2], const int64_t* offsets, int64_t P, int32_t* pair_cell, int32_t* pair_face, void* stream) {
    MOFA_REQUIRE(verts && faces && origin && cell && n && offsets && pair_cell && pair_face, "wind_bin_emit: null pointer");
    MOFA_WIND_COUNT("wind_bin_emit", "F", F);
    MOFA_WIND_COUNT("wind_bin_emit", "V", V);
    MOFA_WIND_COUNT("wind_bin_emit", "P", P);
    WindGrid g;
    MOFA_WIND_GRID("wind_bin_emit");
    MOFA_WIND_LAUNCH(k_wind_bin_emit, F, verts, faces, (long long)F, (int)V, g, offsets, (long long)P, pair_cell, pair_face);
    return check_launch("k_wind_bin_emit");
}

int mofa_wind_query(const float* points, int64_t N, const int64_t* order, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                    int32_t axis, const double origin[2], const double cell[2], const int32_t n[2], const int32_t* cell_start,
                    const int32_t* pair_face, int64_t P, int32_t* winding, int32_t* crossings, int64_t* counts, void* stream) {
    MOFA_REQUIRE(points && verts && faces && origin && cell && n && cell_start && winding && crossings && counts, "wind_query: null pointer");
    MOFA_WIND_COUNT("wind_query", "N", N);
    MOFA_WIND_COUNT("wind_query", "F", F);
    MOFA_WIND_COUNT("wind_query", "V", V);
    MOFA_REQUIRE(P >= 0 && P <= kWindMaxIndex && (pair_face || P == 0), "wind_query: P = %lld (want 0 .. 2^31 - 1, and the pairs unless it is 0)",
                 (long long)P);
    WindGrid g;
    MOFA_WIND_GRID("wind_query");
    MOFA_WIND_LAUNCH(k_wind_query, N, points, (long long)N, order, verts, (int)V, faces, (int)F, cell_start, pair_face, (int)P, g, winding,
                     crossings, counts);
    return check_launch("k_wind_query");
}

}  // extern "C"
