// Mesh ray casting for the geometry export (gfx950): the first or the last hit of many rays on a triangle mesh, through the uniform grid
// of face lists that mofa_dist_bin_count / mofa_dist_bin_emit build (mofa_dist.hip).  mesh.py drives the passes (mesh.ray_cast,
// mesh.ray_bounds); nothing here waits on another thread, no float or double atomic exists (the only atomics are the integer counters),
// and every kernel checks the indices it dereferences: a bad one is skipped, never a fault.
//
//   pair      ray (o, d) against triangle (a, b, c), all the fp32 values widened to fp64, every operation rounded separately (the
//             watertight test of Woop, Benthin and Wald, JCGT 2013):
//               kz = the axis of the largest |d| (a tie: the lowest), kx = (kz + 1) % 3, ky = (kz + 2) % 3, swapped when d[kz] < 0
//               Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
//               X' = X - o;  Xx = X'[kx] - Sx X'[kz], Xy = X'[ky] - Sy X'[kz], Xz = Sz X'[kz]          for X = a, b, c -> A, B, C
//               U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;  some < 0 and some > 0: a miss (zeros are inside)
//               det = (U + V) + W;  det == 0: a miss
//               t = ((U Az + V Bz) + W Cz) / det, then t < zlo ? zlo : t, t > zhi ? zhi : t with zlo / zhi = min / max (Az, Bz, Cz)
//               point[k] = o[k] + t d[k]
//               box rule: tol = 2^-42 (((|o0| + |o1|) + |o2|) + ((m0 + m1) + m2)), m[k] = max(|a[k]|, |b[k]|, |c[k]|); the pair is a miss
//               (counted) when point[k] < min(a, b, c)[k] - tol or point[k] > max(a, b, c)[k] + tol on some axis
//               accepted when t_min <= t <= t_max and the side is not culled (det > 0: front)
//   reduce    the smaller t wins (last: the larger), among equal t the lower face index.  A function of the mesh and the ray alone.
//   walk      per ray, with hi[k] = origin[k] + (double) n[k] cell[k], M[k] = max(|origin[k]|, |hi[k]|),
//             R = ((|o0| + |o1|) + |o2|) + ((M0 + M1) + M2), s[k] = slack[k] + 2^-40 R, Wt = |Sz| s[kz]:
//             the slabs j of cells along kz in ray order (last: reversed); plane(j) = origin[kz] + (double) j cell[kz];
//               Sz > 0:  lo_t = (plane(j) - o[kz]) Sz - Wt,      hi_t = (plane(j + 1) - o[kz]) Sz + Wt
//               Sz < 0:  lo_t = (plane(j + 1) - o[kz]) Sz - Wt,  hi_t = (plane(j) - o[kz]) Sz + Wt
//             first: the walk ends before slab j when (a hit is held and its t < lo_t) or lo_t > t_max;
//             last:  when (a hit is held and its t > hi_t) or hi_t < t_min.
//             ta = max(lo_t, t_min), tb = min(hi_t, t_max); not ta <= tb: the slab is passed over.  Otherwise, for k = kx, ky:
//               pa = o[k] + ta d[k], pb = o[k] + tb d[k];  cells idx(min(pa, pb) - s[k]) .. idx(max(pa, pb) + s[k])  (idx: dist's)
//             and every face listed in a cell of that rectangle of slab j is tested.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kRayMaxIndex = (1ll << 31) - 1;
constexpr double kRayTol = 0x1p-42, kRaySlack = 0x1p-40;

struct RayGrid {
    double origin[3], cell[3], slack[3];
    int n[3];
};

__device__ __forceinline__ bool ray_in_range(int v, int V) { return (unsigned)v < (unsigned)V; }

__device__ __forceinline__ int ray_cell(double x, double origin, double cell, int n) {
    const double t = floor((x - origin) / cell);
    return t >= 0.0 ? (t < (double)n ? (int)t : n - 1) : 0;          // (NaN: 0)
}

__device__ __forceinline__ double ray_pick(const double (&x)[3], int k) { return k == 0 ? x[0] : (k == 1 ? x[1] : x[2]); }

struct Ray {
    double o[3], d[3], Sx, Sy, Sz, abs_o;
    int kx, ky, kz;
};

struct RayHit {
    double t, det, u, v, w;
};

// the header's pair arithmetic: 0 a miss, 1 a hit, 2 a hit that the box rule refuses
__device__ __forceinline__ int ray_triangle(const Ray& r, const double (&a)[3], const double (&b)[3], const double (&c)[3], RayHit& h) {
    const double a_[3] = {a[0] - r.o[0], a[1] - r.o[1], a[2] - r.o[2]}, b_[3] = {b[0] - r.o[0], b[1] - r.o[1], b[2] - r.o[2]},
                 c_[3] = {c[0] - r.o[0], c[1] - r.o[1], c[2] - r.o[2]};
    const double az = ray_pick(a_, r.kz), bz = ray_pick(b_, r.kz), cz = ray_pick(c_, r.kz);
    const double Ax = ray_pick(a_, r.kx) - r.Sx * az, Ay = ray_pick(a_, r.ky) - r.Sy * az, Az = r.Sz * az;
    const double Bx = ray_pick(b_, r.kx) - r.Sx * bz, By = ray_pick(b_, r.ky) - r.Sy * bz, Bz = r.Sz * bz;
    const double Cx = ray_pick(c_, r.kx) - r.Sx * cz, Cy = ray_pick(c_, r.ky) - r.Sy * cz, Cz = r.Sz * cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return 0;
    const double det = (U + V) + W;
    if (det == 0.0 || det != det) return 0;
    double t = ((U * Az + V * Bz) + W * Cz) / det;
    double zlo = Az < Bz ? Az : Bz, zhi = Az > Bz ? Az : Bz;
    zlo = Cz < zlo ? Cz : zlo, zhi = Cz > zhi ? Cz : zhi;
    t = t < zlo ? zlo : t;
    t = t > zhi ? zhi : t;
    const double m0 = fmax(fmax(fabs(a[0]), fabs(b[0])), fabs(c[0])), m1 = fmax(fmax(fabs(a[1]), fabs(b[1])), fabs(c[1])),
                 m2 = fmax(fmax(fabs(a[2]), fabs(b[2])), fabs(c[2]));
    const double tol = kRayTol * (r.abs_o + ((m0 + m1) + m2));
    bool off = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double p = r.o[k] + t * r.d[k];
        const double lo = fmin(fmin(a[k], b[k]), c[k]), hi = fmax(fmax(a[k], b[k]), c[k]);
        off = off || p < lo - tol || p > hi + tol || p != p;
    }
    h.t = t, h.det = det, h.u = U, h.v = V, h.w = W;
    return off ? 2 : 1;
}

__device__ __forceinline__ void ray_wave_add(int64_t* counts, int slot, unsigned long long v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w);
    if (__lane_id() == 0 && v) atomicAdd((unsigned long long*)(counts + slot), v);
}

__global__ __launch_bounds__(256) void k_ray_query(const float* __restrict__ origins, const float* __restrict__ dirs, long long N,
                                                   const int64_t* __restrict__ order, const float* __restrict__ verts, int V,
                                                   const int* __restrict__ faces, int F, const int* __restrict__ cell_start,
                                                   const int* __restrict__ pair_face, int P, RayGrid g, double t_min, double t_max, int last,
                                                   int cull, float* __restrict__ t_out, double* __restrict__ t64_out, int* __restrict__ face_out,
                                                   uint8_t* __restrict__ front_out, float* __restrict__ bary, float* __restrict__ point,
                                                   int64_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long q = -1;
    if (i < N) {
        q = order ? order[i] : i;
        if (q < 0 || q >= N) q = -1;
    }
    unsigned long long tests = 0, off_box = 0;
    int slabs = 0;
    bool bad = false;
    if (q >= 0) {
        const float of[3] = {origins[q * 3 + 0], origins[q * 3 + 1], origins[q * 3 + 2]}, df[3] = {dirs[q * 3 + 0], dirs[q * 3 + 1], dirs[q * 3 + 2]};
        bad = !(isfinite(of[0]) && isfinite(of[1]) && isfinite(of[2]) && isfinite(df[0]) && isfinite(df[1]) && isfinite(df[2])) ||
              (df[0] == 0.0f && df[1] == 0.0f && df[2] == 0.0f);
        int best_face = -1;
        RayHit best;
        best.t = 0.0, best.det = 0.0, best.u = best.v = best.w = 0.0;
        Ray r;
#pragma unroll
        for (int k = 0; k < 3; ++k) r.o[k] = (double)of[k], r.d[k] = (double)df[k];
        if (!bad) {
            const double ad[3] = {fabs(r.d[0]), fabs(r.d[1]), fabs(r.d[2])};
            r.kz = (ad[0] >= ad[1] && ad[0] >= ad[2]) ? 0 : (ad[1] >= ad[2] ? 1 : 2);
            r.kx = (r.kz + 1) % 3, r.ky = (r.kz + 2) % 3;
            const double dz = ray_pick(r.d, r.kz);
            if (dz < 0.0) {
                const int s = r.kx;
                r.kx = r.ky, r.ky = s;
            }
            r.Sx = ray_pick(r.d, r.kx) / dz, r.Sy = ray_pick(r.d, r.ky) / dz, r.Sz = 1.0 / dz;
            r.abs_o = (fabs(r.o[0]) + fabs(r.o[1])) + fabs(r.o[2]);
            double M[3], s[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) M[k] = fmax(fabs(g.origin[k]), fabs(g.origin[k] + (double)g.n[k] * g.cell[k]));
            const double R = r.abs_o + ((M[0] + M[1]) + M[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = g.slack[k] + kRaySlack * R;
            const int kz = r.kz, kx = r.kx, ky = r.ky;
            const int nz = kz == 0 ? g.n[0] : (kz == 1 ? g.n[1] : g.n[2]);
            const double oz = ray_pick(r.o, kz), gz = ray_pick(g.origin, kz), cz = ray_pick(g.cell, kz);
            const double Wt = fabs(r.Sz) * ray_pick(s, kz);
            const bool forward = (r.Sz > 0.0) == (last == 0);
            // strides of the cell id (ix n[1] + iy) n[2] + iz along each axis
            const int stride[3] = {g.n[1] * g.n[2], g.n[2], 1};
            const int sx = kx == 0 ? stride[0] : (kx == 1 ? stride[1] : stride[2]), sy = ky == 0 ? stride[0] : (ky == 1 ? stride[1] : stride[2]),
                      sz = kz == 0 ? stride[0] : (kz == 1 ? stride[1] : stride[2]);
            const int nx = kx == 0 ? g.n[0] : (kx == 1 ? g.n[1] : g.n[2]), ny = ky == 0 ? g.n[0] : (ky == 1 ? g.n[1] : g.n[2]);
            const double ox = ray_pick(r.o, kx), oy = ray_pick(r.o, ky), dx = ray_pick(r.d, kx), dy = ray_pick(r.d, ky);
            const double gx = ray_pick(g.origin, kx), gy = ray_pick(g.origin, ky), cx = ray_pick(g.cell, kx), cy = ray_pick(g.cell, ky);
            const double slx = ray_pick(s, kx), sly = ray_pick(s, ky);
            const long long cells = (long long)g.n[0] * g.n[1] * g.n[2];
            for (int step = 0; step < nz; ++step) {
                const int j = forward ? step : nz - 1 - step;
                const double plo = gz + (double)j * cz, phi = gz + (double)(j + 1) * cz;
                const double e = ((r.Sz > 0.0 ? plo : phi) - oz) * r.Sz, x = ((r.Sz > 0.0 ? phi : plo) - oz) * r.Sz;
                const double lo_t = e - Wt, hi_t = x + Wt;
                if (!last) {
                    if ((best_face >= 0 && best.t < lo_t) || lo_t > t_max) break;
                } else {
                    if ((best_face >= 0 && best.t > hi_t) || hi_t < t_min) break;
                }
                const double ta = lo_t > t_min ? lo_t : t_min, tb = hi_t < t_max ? hi_t : t_max;
                if (!(ta <= tb)) continue;
                ++slabs;
                const double pax = ox + ta * dx, pbx = ox + tb * dx, pay = oy + ta * dy, pby = oy + tb * dy;
                const int x0 = ray_cell((pax < pbx ? pax : pbx) - slx, gx, cx, nx), x1 = ray_cell((pax > pbx ? pax : pbx) + slx, gx, cx, nx);
                const int y0 = ray_cell((pay < pby ? pay : pby) - sly, gy, cy, ny), y1 = ray_cell((pay > pby ? pay : pby) + sly, gy, cy, ny);
                for (int ix = x0; ix <= x1; ++ix)
                    for (int iy = y0; iy <= y1; ++iy) {
                        const long long cid = (long long)ix * sx + (long long)iy * sy + (long long)j * sz;
                        if (cid < 0 || cid >= cells) continue;
                        int j0 = cell_start[cid], j1 = cell_start[cid + 1];
                        j0 = j0 < 0 ? 0 : j0, j1 = j1 > P ? P : j1;
                        for (int p = j0; p < j1; ++p) {
                            const int f = pair_face[p];
                            if (!ray_in_range(f, F)) continue;
                            const int i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
                            if (!ray_in_range(i0, V) || !ray_in_range(i1, V) || !ray_in_range(i2, V)) continue;
                            double a[3], b[3], c[3];
#pragma unroll
                            for (int k = 0; k < 3; ++k)
                                a[k] = (double)verts[(long long)i0 * 3 + k], b[k] = (double)verts[(long long)i1 * 3 + k],
                                c[k] = (double)verts[(long long)i2 * 3 + k];
                            ++tests;
                            RayHit h;
                            const int res = ray_triangle(r, a, b, c, h);
                            if (res == 2) ++off_box;
                            if (res != 1) continue;
                            if (!(h.t >= t_min && h.t <= t_max)) continue;
                            if ((cull == MOFA_RAY_CULL_BACK && h.det < 0.0) || (cull == MOFA_RAY_CULL_FRONT && h.det > 0.0)) continue;
                            const bool better = best_face < 0 || (last ? h.t > best.t : h.t < best.t) || (h.t == best.t && f < best_face);
                            if (better) best = h, best_face = f;
                        }
                    }
            }
        }
        const float nanf_ = __builtin_nanf("");
        const bool hit = best_face >= 0;
        t_out[q] = bad ? nanf_ : (hit ? (float)best.t : __builtin_inff());
        t64_out[q] = bad ? __builtin_nan("") : (hit ? best.t : __builtin_inf());
        face_out[q] = hit ? best_face : -1;
        front_out[q] = hit && best.det > 0.0 ? 1 : 0;
        const double br[3] = {best.u / best.det, best.v / best.det, best.w / best.det};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bary[q * 3 + k] = hit ? (float)br[k] : nanf_;
            point[q * 3 + k] = hit ? (float)(r.o[k] + best.t * r.d[k]) : nanf_;
        }
    }
    ray_wave_add(counts, MOFA_RAY_BAD, bad ? 1ull : 0ull);
    ray_wave_add(counts, MOFA_RAY_TESTS, tests);
    ray_wave_add(counts, MOFA_RAY_OFF_BOX, off_box);
    int m = slabs;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) m = max(m, __shfl_xor(m, w));
    if (__lane_id() == 0 && m > 0) atomicMax((unsigned long long*)(counts + MOFA_RAY_MAX_SLABS), (unsigned long long)m);
}

bool ray_grid(const double* origin, const double* cell, const double* slack, const int32_t* n, RayGrid& g) {
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = origin[a], g.cell[a] = cell[a], g.slack[a] = slack[a], g.n[a] = n[a];
        if (!isfinite(origin[a]) || !isfinite(cell[a]) || !(cell[a] > 0.0) || !isfinite(slack[a]) || !(slack[a] >= 0.0)) return false;
        if (n[a] < 1 || n[a] > MOFA_DIST_MAX_GRID) return false;
        cells *= n[a];
    }
    return cells < kRayMaxIndex;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_RAY_COUNT(name, n) MOFA_REQUIRE((n) >= 1 && (n) <= kRayMaxIndex, "ray_query: " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

extern "C" {

int mofa_ray_query(const float* origins, const float* dirs, int64_t N, const int64_t* order, const float* verts, int64_t V,
                   const int32_t* faces, int64_t F, const double origin[3], const double cell[3], const double slack[3], const int32_t n[3],
                   const int32_t* cell_start, const int32_t* pair_face, int64_t P, double t_min, double t_max, int32_t which, int32_t cull,
                   float* t, double* t64, int32_t* face, uint8_t* front, float* bary, float* point, int64_t* counts, void* stream) {
    MOFA_REQUIRE(origins && dirs && verts && faces && origin && cell && slack && n && cell_start && t && t64 && face && front && bary && point && counts,
                 "ray_query: null pointer");
    MOFA_RAY_COUNT("N", N);
    MOFA_RAY_COUNT("F", F);
    MOFA_RAY_COUNT("V", V);
    MOFA_REQUIRE(P >= 0 && P <= kRayMaxIndex && (pair_face || P == 0), "ray_query: P = %lld (want 0 .. 2^31 - 1, and the pairs unless it is 0)",
                 (long long)P);
    MOFA_REQUIRE(t_min <= t_max, "ray_query: t_min = %g, t_max = %g (want t_min <= t_max, neither NaN)", t_min, t_max);
    MOFA_REQUIRE(which == MOFA_RAY_FIRST || which == MOFA_RAY_LAST, "ray_query: which = %d (want MOFA_RAY_FIRST or MOFA_RAY_LAST)", (int)which);
    MOFA_REQUIRE(cull == MOFA_RAY_CULL_NONE || cull == MOFA_RAY_CULL_BACK || cull == MOFA_RAY_CULL_FRONT, "ray_query: cull = %d (want MOFA_RAY_CULL_*)",
                 (int)cull);
    RayGrid g;
    MOFA_REQUIRE(ray_grid(origin, cell, slack, n, g),
                 "ray_query: origin / cell / slack must be finite, cell > 0, slack >= 0, 1 <= n <= 1024 per axis, fewer than 2^31 - 1 cells");
    hipLaunchKernelGGL(k_ray_query, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, origins, dirs, (long long)N, order, verts, (int)V,
                       faces, (int)F, cell_start, pair_face, (int)P, g, t_min, t_max, which == MOFA_RAY_LAST ? 1 : 0, (int)cull, t, t64, face, front,
                       bary, point, counts);
    return check_launch("k_ray_query");
}

}  // extern "C"
