// Mesh surface distance for the geometry export (gfx950): the exact closest point on a triangle mesh for many query points, through a
// uniform grid of face lists, and a deterministic quadrature of a surface.  mesh.py drives the passes (mesh.closest_points,
// mesh.sample_faces, mesh.surface_distance); nothing here waits on another thread, no float or double atomic exists (the only atomics
// are the integer counters), and every kernel checks the indices it dereferences: a bad one is skipped, never a fault.
//
//   triangle  the closest point of triangle (a, b, c) to p, all four the fp32 coordinates widened to fp64, every operation rounded
//             separately, dot(x, y) = (x0 y0 + x1 y1) + x2 y2, in the region order of Ericson (Real-Time Collision Detection, 5.1.5):
//               ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap);  d1 <= 0 && d2 <= 0             -> A   (1, 0, 0)
//               bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp);                          d3 >= 0 && d4 <= d3            -> B   (0, 1, 0)
//               vc = d1 d4 - d3 d2;   vc <= 0 && d1 >= 0 && d3 <= 0:   v = d1 / (d1 - d3),  q = a + v ab                 -> AB  (1 - v, v, 0)
//               cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp);                          d6 >= 0 && d5 <= d6            -> C   (0, 0, 1)
//               vb = d5 d2 - d1 d6;   vb <= 0 && d2 >= 0 && d6 <= 0:   w = d2 / (d2 - d6),  q = a + w ac                 -> AC  (1 - w, 0, w)
//               va = d3 d6 - d5 d4;   e = d4 - d3, g = d5 - d6;   va <= 0 && e >= 0 && g >= 0:   w = e / (e + g),  q = b + w (c - b)
//                                                                                                                        -> BC  (0, 1 - w, w)
//               s = (va + vb) + vc;   s not finite or s <= 0: the face is skipped for this point (counted);
//               v = vb / s, w = vc / s,  q = (a + v ab) + w ac                                                           -> in  ((1 - v) - w, v, w)
//             then, per axis, q is clamped into [min(a, b, c), max(a, b, c)] (q < lo ? lo : q, then q > hi ? hi : q: the closest point
//             lies in the triangle's box, so this removes rounding only, and the termination bound below leans on it), and
//             d2 = ((px - qx)^2 + (py - qy)^2) + (pz - qz)^2.
//   reduce    across faces the smaller d2 wins, among equal d2 the lower face index; a NaN d2 never wins.  A function of the mesh and
//             the point alone.
//   grid      n = (nx, ny, nz) cells over the box; cell of a coordinate x on an axis: t = floor((x - origin) / cell) in fp64,
//             index = t >= 0 ? (t < n ? (int) t : n - 1) : 0; cell id = (ix ny + iy) nz + iz.  A face whose normal
//             ((aby acz - abz acy), (abz acx - abx acz), (abx acy - aby acx)) is exactly (0, 0, 0) is DEGENERATE: it enters no cell and is
//             counted once; every other face enters each cell of the index box of its three vertices (bin_count / bin_emit).
//   query     from the cell c of the point (clamped as above), the cells of Chebyshev ring r = 0, 1, 2, ... (clipped to the grid); after
//             ring r, for every side of the visited block that has not reached the grid's edge (c - r > 0, c + r < n - 1):
//               low:  ((p - (origin + (double)(c - r) cell)) - slack) shrink       high:  (((origin + (double)(c + r + 1) cell) - p) - slack) shrink
//             lb = the smallest of them (shrink = 1 - 2^-40).  The walk ends when no such side is left, or when lb > 0 and
//             (best d2 < lb lb  or  lb > max_distance).
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kDistMaxIndex = (1ll << 31) - 1;     // N, V, F, the pair count and the cell count: int32 indices
constexpr double kDistShrink = 1.0 - 0x1p-40;

struct DistGrid {
    double origin[3], cell[3], slack[3];
    int n[3];
};

__device__ __forceinline__ bool dist_in_range(int v, int V) { return (unsigned)v < (unsigned)V; }

__device__ __forceinline__ double dist_dot(const double (&x)[3], const double (&y)[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__device__ __forceinline__ int dist_cell(double x, double origin, double cell, int n) {
    const double t = floor((x - origin) / cell);
    return t >= 0.0 ? (t < (double)n ? (int)t : n - 1) : 0;          // (NaN: 0)
}

__device__ __forceinline__ void dist_load(const float* __restrict__ verts, int i, double (&p)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (double)verts[(long long)i * 3 + c];
}

__device__ __forceinline__ bool dist_zero_normal(const double (&a)[3], const double (&b)[3], const double (&c)[3], double (&n)[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = ab[1] * ac[2] - ab[2] * ac[1], n[1] = ab[2] * ac[0] - ab[0] * ac[2], n[2] = ab[0] * ac[1] - ab[1] * ac[0];
    return n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0;
}

struct DistHit {
    double d2, q[3], bary[3];
};

// the header's point-triangle arithmetic; false: the interior was reached with an unusable s (the face is skipped for this point)
__device__ __forceinline__ bool dist_triangle(const double (&p)[3], const double (&a)[3], const double (&b)[3], const double (&c)[3], DistHit& h) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double d1 = dist_dot(ab, ap), d2 = dist_dot(ac, ap);
    bool done = false;
    if (d1 <= 0.0 && d2 <= 0.0) {
        h.q[0] = a[0], h.q[1] = a[1], h.q[2] = a[2], h.bary[0] = 1.0, h.bary[1] = 0.0, h.bary[2] = 0.0, done = true;
    }
    double d3 = 0.0, d4 = 0.0, d5 = 0.0, d6 = 0.0;
    if (!done) {
        const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
        d3 = dist_dot(ab, bp), d4 = dist_dot(ac, bp);
        if (d3 >= 0.0 && d4 <= d3) {
            h.q[0] = b[0], h.q[1] = b[1], h.q[2] = b[2], h.bary[0] = 0.0, h.bary[1] = 1.0, h.bary[2] = 0.0, done = true;
        }
    }
    double vc = 0.0;
    if (!done) {
        vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double v = d1 / (d1 - d3);
#pragma unroll
            for (int k = 0; k < 3; ++k) h.q[k] = a[k] + v * ab[k];
            h.bary[0] = 1.0 - v, h.bary[1] = v, h.bary[2] = 0.0, done = true;
        }
    }
    if (!done) {
        const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
        d5 = dist_dot(ab, cp), d6 = dist_dot(ac, cp);
        if (d6 >= 0.0 && d5 <= d6) {
            h.q[0] = c[0], h.q[1] = c[1], h.q[2] = c[2], h.bary[0] = 0.0, h.bary[1] = 0.0, h.bary[2] = 1.0, done = true;
        }
    }
    double vb = 0.0;
    if (!done) {
        vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
#pragma unroll
            for (int k = 0; k < 3; ++k) h.q[k] = a[k] + w * ac[k];
            h.bary[0] = 1.0 - w, h.bary[1] = 0.0, h.bary[2] = w, done = true;
        }
    }
    if (!done) {
        const double va = d3 * d6 - d5 * d4, e = d4 - d3, g = d5 - d6;
        if (va <= 0.0 && e >= 0.0 && g >= 0.0) {
            const double w = e / (e + g);
#pragma unroll
            for (int k = 0; k < 3; ++k) h.q[k] = b[k] + w * (c[k] - b[k]);
            h.bary[0] = 0.0, h.bary[1] = 1.0 - w, h.bary[2] = w;
        } else {
            const double s = (va + vb) + vc;
            if (!(isfinite(s) && s > 0.0)) return false;
            const double v = vb / s, w = vc / s;
#pragma unroll
            for (int k = 0; k < 3; ++k) h.q[k] = (a[k] + v * ab[k]) + w * ac[k];
            h.bary[0] = (1.0 - v) - w, h.bary[1] = v, h.bary[2] = w;
        }
    }
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double lo = a[k] < b[k] ? a[k] : b[k], hi = a[k] > b[k] ? a[k] : b[k];
        lo = c[k] < lo ? c[k] : lo, hi = c[k] > hi ? c[k] : hi;
        double q = h.q[k];
        q = q < lo ? lo : q;
        q = q > hi ? hi : q;
        h.q[k] = q;
        d[k] = p[k] - q;
    }
    h.d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    return true;
}

// sums `v` over the wavefront (every lane of it must call) and adds the total to counts[slot]: one integer atomic per wavefront
__device__ __forceinline__ void dist_wave_add(int64_t* counts, int slot, unsigned long long v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w);
    if (__lane_id() == 0 && v) atomicAdd((unsigned long long*)(counts + slot), v);
}

__global__ __launch_bounds__(256) void k_dist_validate(const float* __restrict__ verts, long long n, int64_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool bad = i < n && !isfinite(verts[i]);
    const unsigned long long b = __ballot(bad);
    if (bad && (int)__lane_id() == __ffsll(b) - 1) atomicAdd((unsigned long long*)counts, (unsigned long long)__popcll(b));
}

// the index box of a face, false for a face that enters no cell (a bad index, a zero normal)
__device__ __forceinline__ bool dist_face_box(const float* __restrict__ verts, const int* __restrict__ faces, long long f, int V, const DistGrid& g,
                                              int (&lo)[3], int (&hi)[3], bool& degenerate) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    degenerate = false;
    if (!dist_in_range(i0, V) || !dist_in_range(i1, V) || !dist_in_range(i2, V)) return false;
    double a[3], b[3], c[3], n[3];
    dist_load(verts, i0, a), dist_load(verts, i1, b), dist_load(verts, i2, c);
    if (dist_zero_normal(a, b, c, n)) {
        degenerate = true;
        return false;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ca = dist_cell(a[k], g.origin[k], g.cell[k], g.n[k]), cb = dist_cell(b[k], g.origin[k], g.cell[k], g.n[k]),
                  cc = dist_cell(c[k], g.origin[k], g.cell[k], g.n[k]);
        lo[k] = min(ca, min(cb, cc)), hi[k] = max(ca, max(cb, cc));
    }
    return true;
}

__global__ __launch_bounds__(256) void k_dist_bin_count(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V, DistGrid g,
                                                        int64_t* __restrict__ n_cells, int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool degenerate = false;
    if (f < F) {
        int lo[3], hi[3];
        long long n = 0;
        if (dist_face_box(verts, faces, f, V, g, lo, hi, degenerate)) n = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
        n_cells[f] = n;
    }
    const unsigned long long b = __ballot(degenerate);
    if (degenerate && (int)__lane_id() == __ffsll(b) - 1)
        atomicAdd((unsigned long long*)(counts + MOFA_DIST_DEGENERATE), (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(256) void k_dist_bin_emit(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V, DistGrid g,
                                                       const int64_t* __restrict__ offsets, long long P, int* __restrict__ pair_cell,
                                                       int* __restrict__ pair_face) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int lo[3], hi[3];
    bool degenerate;
    if (!dist_face_box(verts, faces, f, V, g, lo, hi, degenerate)) return;
    long long o = offsets[f];
    for (int ix = lo[0]; ix <= hi[0]; ++ix)
        for (int iy = lo[1]; iy <= hi[1]; ++iy)
            for (int iz = lo[2]; iz <= hi[2]; ++iz, ++o) {
                if (o < 0 || o >= P) return;                                     // (offsets that do not belong to this mesh and grid)
                pair_cell[o] = (ix * g.n[1] + iy) * g.n[2] + iz;
                pair_face[o] = (int)f;
            }
}

struct DistBest {
    double d2, q[3], bary[3];
    int face;
};

// the faces of the cells first .. last (consecutive ids: one run of the sorted pairs)
__device__ __forceinline__ void dist_visit(const double (&p)[3], const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                           const int* __restrict__ cell_start, const int* __restrict__ pair_face, int P, int first, int last,
                                           DistBest& best, unsigned long long& tests, unsigned long long& skipped) {
    int j0 = cell_start[first], j1 = cell_start[last + 1];
    j0 = j0 < 0 ? 0 : j0, j1 = j1 > P ? P : j1;
    for (int j = j0; j < j1; ++j) {
        const int f = pair_face[j];
        if (!dist_in_range(f, F)) continue;
        const int i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
        if (!dist_in_range(i0, V) || !dist_in_range(i1, V) || !dist_in_range(i2, V)) continue;
        double a[3], b[3], c[3];
        dist_load(verts, i0, a), dist_load(verts, i1, b), dist_load(verts, i2, c);
        ++tests;
        DistHit h;
        if (!dist_triangle(p, a, b, c, h)) {
            ++skipped;
            continue;
        }
        if (h.d2 < best.d2 || (h.d2 == best.d2 && f < best.face)) {
            best.d2 = h.d2, best.face = f;
#pragma unroll
            for (int k = 0; k < 3; ++k) best.q[k] = h.q[k], best.bary[k] = h.bary[k];
        }
    }
}

__global__ __launch_bounds__(256) void k_dist_query(const float* __restrict__ points, long long N, const int64_t* __restrict__ order,
                                                    const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                    const int* __restrict__ cell_start, const int* __restrict__ pair_face, int P, DistGrid g,
                                                    double max_distance, float* __restrict__ distance, double* __restrict__ d2_out,
                                                    int* __restrict__ face_out, float* __restrict__ closest, float* __restrict__ bary,
                                                    int64_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long q = -1;
    if (i < N) {
        q = order ? order[i] : i;
        if (q < 0 || q >= N) q = -1;
    }
    unsigned long long tests = 0, skipped = 0;
    int ring = 0;
    bool non_finite = false;
    if (q >= 0) {
        const float pf[3] = {points[q * 3 + 0], points[q * 3 + 1], points[q * 3 + 2]};
        const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        const float nanf_ = __builtin_nanf("");
        DistBest best;
        best.d2 = __builtin_inf(), best.face = -1;
        non_finite = !(isfinite(pf[0]) && isfinite(pf[1]) && isfinite(pf[2]));
        if (!non_finite) {
            const int c[3] = {dist_cell(p[0], g.origin[0], g.cell[0], g.n[0]), dist_cell(p[1], g.origin[1], g.cell[1], g.n[1]),
                              dist_cell(p[2], g.origin[2], g.cell[2], g.n[2])};
            for (int r = 0;; ++r) {
                ring = r;
                const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.n[0] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
                const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1);
                for (int ix = x0; ix <= x1; ++ix) {
                    const bool fx = ix == c[0] - r || ix == c[0] + r;
                    for (int iy = y0; iy <= y1; ++iy) {
                        const int row = (ix * g.n[1] + iy) * g.n[2];
                        if (fx || iy == c[1] - r || iy == c[1] + r) {
                            dist_visit(p, verts, V, faces, F, cell_start, pair_face, P, row + z0, row + z1, best, tests, skipped);
                        } else {                                                           // (r > 0 here: the two ends of the row)
                            if (c[2] - r >= 0) dist_visit(p, verts, V, faces, F, cell_start, pair_face, P, row + c[2] - r, row + c[2] - r, best, tests, skipped);
                            if (c[2] + r <= g.n[2] - 1)
                                dist_visit(p, verts, V, faces, F, cell_start, pair_face, P, row + c[2] + r, row + c[2] + r, best, tests, skipped);
                        }
                    }
                }
                bool open = false;
                double lb = __builtin_inf();
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int lo = c[k] - r, hi = c[k] + r;
                    if (lo > 0) {
                        const double d = ((p[k] - (g.origin[k] + (double)lo * g.cell[k])) - g.slack[k]) * kDistShrink;
                        lb = d < lb ? d : lb, open = true;
                    }
                    if (hi < g.n[k] - 1) {
                        const double d = (((g.origin[k] + (double)(hi + 1) * g.cell[k]) - p[k]) - g.slack[k]) * kDistShrink;
                        lb = d < lb ? d : lb, open = true;
                    }
                }
                if (!open) break;
                if (lb > 0.0 && (best.d2 < lb * lb || lb > max_distance)) break;
            }
        }
        const double d = sqrt(best.d2);
        const bool hit = !non_finite && best.face >= 0 && d <= max_distance;
        distance[q] = non_finite ? nanf_ : (hit ? (float)d : __builtin_inff());
        d2_out[q] = non_finite ? __builtin_nan("") : (hit ? best.d2 : __builtin_inf());
        face_out[q] = hit ? best.face : -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            closest[q * 3 + k] = hit ? (float)best.q[k] : nanf_;
            bary[q * 3 + k] = hit ? (float)best.bary[k] : nanf_;
        }
    }
    dist_wave_add(counts, MOFA_DIST_NON_FINITE, non_finite ? 1ull : 0ull);
    dist_wave_add(counts, MOFA_DIST_TESTS, tests);
    dist_wave_add(counts, MOFA_DIST_SKIPPED, skipped);
    int m = ring;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) m = max(m, __shfl_xor(m, w));
    if (__lane_id() == 0 && m > 0) atomicMax((unsigned long long*)(counts + MOFA_DIST_MAX_RING), (unsigned long long)m);
}

__global__ __launch_bounds__(256) void k_dist_sample_count(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V,
                                                           double spacing, int max_subdiv, double* __restrict__ area, int* __restrict__ k_out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    double ar = 0.0;
    int kf = 0;
    if (dist_in_range(i0, V) && dist_in_range(i1, V) && dist_in_range(i2, V)) {
        double a[3], b[3], c[3], n[3];
        dist_load(verts, i0, a), dist_load(verts, i1, b), dist_load(verts, i2, c);
        if (!dist_zero_normal(a, b, c, n)) {
            ar = 0.5 * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]},
                         bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
            double l2 = dist_dot(ab, ab);
            const double l2ac = dist_dot(ac, ac), l2bc = dist_dot(bc, bc);
            l2 = l2ac > l2 ? l2ac : l2, l2 = l2bc > l2 ? l2bc : l2;
            const double t = ceil(sqrt(l2) / spacing);
            kf = t >= 1.0 ? (t < (double)max_subdiv ? (int)t : max_subdiv) : 1;       // (NaN: 1)
        }
    }
    area[f] = ar, k_out[f] = kf;
}

__global__ __launch_bounds__(256) void k_dist_sample_emit(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V,
                                                          const double* __restrict__ area, const int* __restrict__ kf, const int64_t* __restrict__ offsets,
                                                          const int* __restrict__ face_of, long long S, float* __restrict__ points,
                                                          double* __restrict__ weight) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const float nanf_ = __builtin_nanf("");
    points[s * 3 + 0] = points[s * 3 + 1] = points[s * 3 + 2] = nanf_, weight[s] = 0.0;       // what a sample that matches no face keeps
    const int f = face_of[s];
    if ((unsigned)f >= (unsigned long long)F) return;
    const int k = kf[f];
    const long long t = s - offsets[f];
    if (k < 1 || k > MOFA_DIST_MAX_SUBDIV || t < 0 || t >= (long long)k * k) return;
    const int i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
    if (!dist_in_range(i0, V) || !dist_in_range(i1, V) || !dist_in_range(i2, V)) return;
    // row i holds 2 (k - i) - 1 sub-triangles and starts at 2 k i - i^2
    int i = 0;
    while (i + 1 < k && 2ll * k * (i + 1) - (long long)(i + 1) * (i + 1) <= t) ++i;
    const int r = (int)(t - (2ll * k * i - (long long)i * i)), j = r >> 1, inv = r & 1;
    const int nv = 3 * i + 1 + inv, nw = 3 * j + 1 + inv, nu = 3 * k - nv - nw;
    double a[3], b[3], c[3];
    dist_load(verts, i0, a), dist_load(verts, i1, b), dist_load(verts, i2, c);
    const double du = (double)nu, dv = (double)nv, dw = (double)nw, den = (double)(3 * k);
#pragma unroll
    for (int x = 0; x < 3; ++x) points[s * 3 + x] = (float)(((du * a[x] + dv * b[x]) + dw * c[x]) / den);
    weight[s] = area[f] / (double)(k * k);
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

bool dist_grid(const double* origin, const double* cell, const double* slack, const int32_t* n, DistGrid& g) {
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = origin[a], g.cell[a] = cell[a], g.slack[a] = slack[a], g.n[a] = n[a];
        if (!isfinite(origin[a]) || !isfinite(cell[a]) || !(cell[a] > 0.0) || !isfinite(slack[a]) || !(slack[a] >= 0.0)) return false;
        if (n[a] < 1 || n[a] > MOFA_DIST_MAX_GRID) return false;
        cells *= n[a];
    }
    return cells < kDistMaxIndex;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_DIST_COUNT(what, name, n) \
    MOFA_REQUIRE((n) >= 1 && (n) <= kDistMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))
#define MOFA_DIST_GRID(what) \
    MOFA_REQUIRE(dist_grid(origin, cell, slack, n, g), what ": origin / cell / slack must be finite, cell > 0, slack >= 0, 1 <= n <= 1024 per axis, fewer than 2^31 - 1 cells")

extern "C" {

int mofa_dist_validate(const float* verts, int64_t V, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts && counts, "dist_validate: null pointer");
    MOFA_DIST_COUNT("dist_validate", "V", V);
    hipLaunchKernelGGL(k_dist_validate, dim3(blocks_of(3 * V)), dim3(256), 0, (hipStream_t)stream, verts, (long long)(3 * V), counts);
    return check_launch("k_dist_validate");
}

int mofa_dist_bin_count(const float* verts, const int32_t* faces, int64_t F, int64_t V, const double origin[3], const double cell[3],
                        const double slack[3], const int32_t n[3], int64_t* n_cells, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts && faces && origin && cell && slack && n && n_cells && counts, "dist_bin_count: null pointer");
    MOFA_DIST_COUNT("dist_bin_count", "F", F);
    MOFA_DIST_COUNT("dist_bin_count", "V", V);
    DistGrid g;
    MOFA_DIST_GRID("dist_bin_count");
    hipLaunchKernelGGL(k_dist_bin_count, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, g, n_cells, counts);
    return check_launch("k_dist_bin_count");
}

int mofa_dist_bin_emit(const float* verts, const int32_t* faces, int64_t F, int64_t V, const double origin[3], const double cell[3],
                       const double slack[3], const int32_t n[3], const int64_t* offsets, int64_t P, int32_t* pair_cell, int32_t* pair_face,
                       void* stream) {
    MOFA_REQUIRE(verts && faces && origin && cell && slack && n && offsets && pair_cell && pair_face, "dist_bin_emit: null pointer");
    MOFA_DIST_COUNT("dist_bin_emit", "F", F);
    MOFA_DIST_COUNT("dist_bin_emit", "V", V);
    MOFA_DIST_COUNT("dist_bin_emit", "P", P);
    DistGrid g;
    MOFA_DIST_GRID("dist_bin_emit");
    hipLaunchKernelGGL(k_dist_bin_emit, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, g, offsets,
                       (long long)P, pair_cell, pair_face);
    return check_launch("k_dist_bin_emit");
}

int mofa_dist_query(const float* points, int64_t N, const int64_t* order, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                    const double origin[3], const double cell[3], const double slack[3], const int32_t n[3], const int32_t* cell_start,
                    const int32_t* pair_face, int64_t P, double max_distance, float* distance, double* d2, int32_t* face, float* closest,
                    float* bary, int64_t* counts, void* stream) {
    MOFA_REQUIRE(points && verts && faces && origin && cell && slack && n && cell_start && distance && d2 && face && closest && bary && counts,
                 "dist_query: null pointer");
    MOFA_DIST_COUNT("dist_query", "N", N);
    MOFA_DIST_COUNT("dist_query", "F", F);
    MOFA_DIST_COUNT("dist_query", "V", V);
    MOFA_REQUIRE(P >= 0 && P <= kDistMaxIndex && (pair_face || P == 0), "dist_query: P = %lld (want 0 .. 2^31 - 1, and the pairs unless it is 0)",
                 (long long)P);
    MOFA_REQUIRE(max_distance > 0.0, "dist_query: max_distance = %g (want > 0; infinity means unbounded)", max_distance);
    DistGrid g;
    MOFA_DIST_GRID("dist_query");
    hipLaunchKernelGGL(k_dist_query, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, points, (long long)N, order, verts, (int)V, faces, (int)F,
                       cell_start, pair_face, (int)P, g, max_distance, distance, d2, face, closest, bary, counts);
    return check_launch("k_dist_query");
}

int mofa_dist_sample_count(const float* verts, const int32_t* faces, int64_t F, int64_t V, double spacing, int32_t max_subdiv, double* area,
                           int32_t* k, void* stream) {
    MOFA_REQUIRE(verts && faces && area && k, "dist_sample_count: null pointer");
    MOFA_DIST_COUNT("dist_sample_count", "F", F);
    MOFA_DIST_COUNT("dist_sample_count", "V", V);
    MOFA_REQUIRE(isfinite(spacing) && spacing > 0.0, "dist_sample_count: spacing = %g (want finite and > 0)", spacing);
    MOFA_REQUIRE(max_subdiv >= 1 && max_subdiv <= MOFA_DIST_MAX_SUBDIV, "dist_sample_count: max_subdiv = %d (want 1 .. %d)", (int)max_subdiv,
                 MOFA_DIST_MAX_SUBDIV);
    hipLaunchKernelGGL(k_dist_sample_count, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, spacing,
                       (int)max_subdiv, area, k);
    return check_launch("k_dist_sample_count");
}

int mofa_dist_sample_emit(const float* verts, const int32_t* faces, int64_t F, int64_t V, const double* area, const int32_t* k,
                          const int64_t* offsets, const int32_t* face_of, int64_t S, float* points, double* weight, void* stream) {
    MOFA_REQUIRE(verts && faces && area && k && offsets && face_of && points && weight, "dist_sample_emit: null pointer");
    MOFA_DIST_COUNT("dist_sample_emit", "F", F);
    MOFA_DIST_COUNT("dist_sample_emit", "V", V);
    MOFA_DIST_COUNT("dist_sample_emit", "S", S);
    hipLaunchKernelGGL(k_dist_sample_emit, dim3(blocks_of(S)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, area, k, offsets,
                       face_of, (long long)S, points, weight);
    return check_launch("k_dist_sample_emit");
}

}  // extern "C"
