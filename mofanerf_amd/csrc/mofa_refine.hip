// Vertex refinement for the geometry export (gfx950): every vertex of mofa_iso_emit / mofa_band_emit keeps its lattice edge and moves
// along it by a bracketed bisection on densities the caller supplies, and density normals come from central differences of the same
// densities.  Nothing here evaluates the network: the kernels make sample points and consume densities, one thread per vertex.
//
//   edge       edge_id = 7 idx + dir (mofa_lattice.h); p_a, p_b = grid_coord per axis at its lower / upper end: mofa_grid_points' bits
//   bracket    (t_lo, s_lo), (t_hi, s_hi): two parameters on the edge whose densities lie on different sides of the level; starts (0, s_a), (1, s_b)
//   midpoint   t_m = 0.5 (t_lo + t_hi) (exact for 23 halvings), p = p_a + t_m (p_b - p_a)
//   update     inside(s_m) == inside(s_lo) ? (t_lo, s_lo) = (t_m, s_m) : (t_hi, s_hi) = (t_m, s_m)
//   place      u = (level - s_lo) / (s_hi - s_lo), t = t_lo + u (t_hi - t_lo), p = p_a + t (p_b - p_a): with the bracket untouched t = u, the
//              vertex of k_iso_vertices bit for bit
//   normals    g_a = (s(v + h_a e_a) - s(v - h_a e_a)) / (2 h_a) in fp32; n = -g / |g|, norm and division in fp64, rounded once
//
// Every fp32 operation is rounded separately.  The only atomics are the error counters (words of counts[MOFA_REFINE_COUNTS], which the
// caller zeroes and the kernels add to): the same input gives the same bits.
#include <math.h>

#include "mofa_common.h"
#include "mofa_lattice.h"

namespace mofa {
namespace {

constexpr long long kRefineMaxAxis = 1ll << 24;       // (float)i is exact: the grid_coord formula holds

struct Lattice {
    long long nx, ny, nz;
    float lo[3], step[3];
};

__device__ __forceinline__ void count_one(int64_t* counts, int word) { atomicAdd((unsigned long long*)(counts + word), 1ull); }

// the two ends of edge `e` as lattice indices; false for an id outside the grid or an edge that leaves it
__device__ __forceinline__ bool edge_ends(const Lattice& g, long long e, long long (&a)[3], long long (&b)[3]) {
    if (e < 0 || e >= 7 * g.nx * g.ny * g.nz) return false;
    const long long idx = e / 7;
    const int dir = (int)(e - idx * 7);
    a[0] = idx / (g.ny * g.nz);
    const long long r = idx - a[0] * (g.ny * g.nz);
    a[1] = r / g.nz;
    a[2] = r - a[1] * g.nz;
    b[0] = a[0] + kDirDx[dir], b[1] = a[1] + kDirDy[dir], b[2] = a[2] + kDirDz[dir];
    return b[0] < g.nx && b[1] < g.ny && b[2] < g.nz;
}

__device__ __forceinline__ float bracket_mid(float t_lo, float t_hi) { return __fmul_rn(0.5f, __fadd_rn(t_lo, t_hi)); }

// p = p_a + t (p_b - p_a) on the edge with ends a, b
__device__ __forceinline__ void edge_point(const Lattice& g, const long long (&a)[3], const long long (&b)[3], float t, float* __restrict__ p) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pa = grid_coord(g.lo[c], g.step[c], a[c]), pb = grid_coord(g.lo[c], g.step[c], b[c]);
        p[c] = __fadd_rn(pa, __fmul_rn(t, __fsub_rn(pb, pa)));
    }
}

// pts[t] for vertex first + t: mode 0 = p_a, 1 = p_b, 2 = the bracket's midpoint
__global__ __launch_bounds__(256) void k_edge_points(Lattice g, const int64_t* __restrict__ edge_ids, const float* __restrict__ t_lo,
                                                     const float* __restrict__ t_hi, long long first, long long n, int mode,
                                                     float* __restrict__ pts, int64_t* __restrict__ counts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long long v = first + t;
    long long a[3], b[3];
    if (!edge_ends(g, edge_ids[v], a, b)) {
        count_one(counts, MOFA_REFINE_REFUSED);
        return;
    }
    if (mode == 2) {
        edge_point(g, a, b, bracket_mid(t_lo[v], t_hi[v]), pts + t * 3);
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[t * 3 + c] = grid_coord(g.lo[c], g.step[c], mode == 0 ? a[c] : b[c]);
}

__global__ __launch_bounds__(256) void k_edge_bracket_init(const float* __restrict__ s_a, const float* __restrict__ s_b, float level, long long n,
                                                           float* __restrict__ t_lo, float* __restrict__ t_hi, float* __restrict__ s_lo,
                                                           float* __restrict__ s_hi, int64_t* __restrict__ counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const float a = s_a[v], b = s_b[v];
    t_lo[v] = 0.f, t_hi[v] = 1.f, s_lo[v] = a, s_hi[v] = b;
    if (inside(a, level) == inside(b, level)) count_one(counts, MOFA_REFINE_NO_STRADDLE);
    if (!isfinite(a)) count_one(counts, MOFA_REFINE_NON_FINITE);
    if (!isfinite(b)) count_one(counts, MOFA_REFINE_NON_FINITE);
}

__global__ __launch_bounds__(256) void k_edge_bracket_update(const float* __restrict__ s_m, float level, long long n, float* __restrict__ t_lo,
                                                             float* __restrict__ t_hi, float* __restrict__ s_lo, float* __restrict__ s_hi,
                                                             int64_t* __restrict__ counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const float m = s_m[v];
    if (!isfinite(m)) {
        count_one(counts, MOFA_REFINE_NON_FINITE);
        return;
    }
    const float t_m = bracket_mid(t_lo[v], t_hi[v]);
    if (inside(m, level) == inside(s_lo[v], level)) t_lo[v] = t_m, s_lo[v] = m;
    else t_hi[v] = t_m, s_hi[v] = m;
}

__global__ __launch_bounds__(256) void k_edge_place(Lattice g, const int64_t* __restrict__ edge_ids, const float* __restrict__ t_lo,
                                                    const float* __restrict__ t_hi, const float* __restrict__ s_lo,
                                                    const float* __restrict__ s_hi, float level, long long n, float* __restrict__ verts,
                                                    int64_t* __restrict__ counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    long long a[3], b[3];
    if (!edge_ends(g, edge_ids[v], a, b)) {
        count_one(counts, MOFA_REFINE_REFUSED);
        return;
    }
    const float u = __fdiv_rn(__fsub_rn(level, s_lo[v]), __fsub_rn(s_hi[v], s_lo[v]));
    const float t = __fadd_rn(t_lo[v], __fmul_rn(u, __fsub_rn(t_hi[v], t_lo[v])));
    edge_point(g, a, b, t, verts + v * 3);
}

// pts[6 t + q] for vertex first + t: q = 0 .. 5 is +x, -x, +y, -y, +z, -z
__global__ __launch_bounds__(256) void k_fd_points(const float* __restrict__ verts, float hx, float hy, float hz, long long first, long long n,
                                                   float* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float h[3] = {hx, hy, hz};
    const float* p = verts + (first + t) * 3;
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            pts[(t * 6 + q) * 3 + c] = c != (q >> 1) ? p[c] : ((q & 1) ? __fsub_rn(p[c], h[c]) : __fadd_rn(p[c], h[c]));
}

__global__ __launch_bounds__(256) void k_fd_normals(const float* __restrict__ s, float hx, float hy, float hz, long long n,
                                                    float* __restrict__ normals, int64_t* __restrict__ counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const float h[3] = {hx, hy, hz};
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = __fdiv_rn(__fsub_rn(s[v * 6 + 2 * c], s[v * 6 + 2 * c + 1]), __fmul_rn(2.f, h[c]));
    const double gx = (double)g[0], gy = (double)g[1], gz = (double)g[2];
    const double norm = sqrt(gx * gx + gy * gy + gz * gz);
    const bool ok = isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && norm > 0.0;
    if (!ok) count_one(counts, MOFA_REFINE_ZERO_NORMAL);
    normals[v * 3 + 0] = ok ? (float)(-gx / norm) : 0.f;
    normals[v * 3 + 1] = ok ? (float)(-gy / norm) : 0.f;
    normals[v * 3 + 2] = ok ? (float)(-gz / norm) : 0.f;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }
constexpr long long kMaxLaunch = (1ll << 31) * 256 - 256;      // one thread per element, at most 2^31 - 1 workgroups

int lattice_of(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], const char* what, Lattice& g) {
    MOFA_REQUIRE(lo && step, "%s: null pointer", what);
    MOFA_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && nx < kRefineMaxAxis && ny < kRefineMaxAxis && nz < kRefineMaxAxis && nx * ny < (1ll << 40) &&
                     nx * ny * nz < (1ll << 48),
                 "%s: grid %lld x %lld x %lld (want 2 <= n < 2^24 per axis and fewer than 2^48 samples)", what, (long long)nx, (long long)ny,
                 (long long)nz);
    for (int a = 0; a < 3; ++a)
        MOFA_REQUIRE(isfinite(lo[a]) && isfinite(step[a]) && step[a] > 0.f, "%s: lo[%d] = %g, step[%d] = %g (want finite, step > 0)", what, a,
                     (double)lo[a], a, (double)step[a]);
    g = Lattice{nx, ny, nz, {lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}};
    return MOFA_OK;
}

int spacing_check(const float h[3], const char* what) {
    MOFA_REQUIRE(h, "%s: null pointer", what);
    for (int a = 0; a < 3; ++a) MOFA_REQUIRE(isfinite(h[a]) && h[a] > 0.f, "%s: h[%d] = %g (want finite and > 0)", what, a, (double)h[a]);
    return MOFA_OK;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_REFINE_RANGE(what) \
    MOFA_REQUIRE(n > 0 && n <= kMaxLaunch, what ": n = %lld (want 1 .. 2^39 - 256)", (long long)n)

extern "C" {

int mofa_edge_points(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], const int64_t* edge_ids, const float* t_lo,
                     const float* t_hi, int64_t first, int64_t n, int32_t mode, float* pts, int64_t* counts, void* stream) {
    Lattice g;
    const int rc = lattice_of(nx, ny, nz, lo, step, "edge_points", g);
    if (rc != MOFA_OK) return rc;
    MOFA_REQUIRE(edge_ids && pts && counts, "edge_points: null pointer");
    MOFA_REQUIRE(mode >= 0 && mode <= 2, "edge_points: mode = %d (0: lower end, 1: upper end, 2: the bracket's midpoint)", (int)mode);
    MOFA_REQUIRE(mode != 2 || (t_lo && t_hi), "edge_points: the midpoint needs t_lo and t_hi");
    MOFA_REFINE_RANGE("edge_points");
    MOFA_REQUIRE(first >= 0 && first <= (1ll << 62), "edge_points: first = %lld", (long long)first);
    hipLaunchKernelGGL(k_edge_points, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, g, edge_ids, t_lo, t_hi, (long long)first,
                       (long long)n, (int)mode, pts, counts);
    return check_launch("k_edge_points");
}

int mofa_edge_bracket_init(const float* s_a, const float* s_b, float level, int64_t n, float* t_lo, float* t_hi, float* s_lo, float* s_hi,
                           int64_t* counts, void* stream) {
    MOFA_REQUIRE(s_a && s_b && t_lo && t_hi && s_lo && s_hi && counts, "edge_bracket_init: null pointer");
    MOFA_REQUIRE(isfinite(level), "edge_bracket_init: the level must be finite (got %g)", (double)level);
    MOFA_REFINE_RANGE("edge_bracket_init");
    hipLaunchKernelGGL(k_edge_bracket_init, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, s_a, s_b, level, (long long)n, t_lo, t_hi,
                       s_lo, s_hi, counts);
    return check_launch("k_edge_bracket_init");
}

int mofa_edge_bracket_update(const float* s_m, float level, int64_t n, float* t_lo, float* t_hi, float* s_lo, float* s_hi, int64_t* counts,
                             void* stream) {
    MOFA_REQUIRE(s_m && t_lo && t_hi && s_lo && s_hi && counts, "edge_bracket_update: null pointer");
    MOFA_REQUIRE(isfinite(level), "edge_bracket_update: the level must be finite (got %g)", (double)level);
    MOFA_REFINE_RANGE("edge_bracket_update");
    hipLaunchKernelGGL(k_edge_bracket_update, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, s_m, level, (long long)n, t_lo, t_hi, s_lo,
                       s_hi, counts);
    return check_launch("k_edge_bracket_update");
}

int mofa_edge_place(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], const int64_t* edge_ids, const float* t_lo,
                    const float* t_hi, const float* s_lo, const float* s_hi, float level, int64_t n, float* verts, int64_t* counts,
                    void* stream) {
    Lattice g;
    const int rc = lattice_of(nx, ny, nz, lo, step, "edge_place", g);
    if (rc != MOFA_OK) return rc;
    MOFA_REQUIRE(edge_ids && t_lo && t_hi && s_lo && s_hi && verts && counts, "edge_place: null pointer");
    MOFA_REQUIRE(isfinite(level), "edge_place: the level must be finite (got %g)", (double)level);
    MOFA_REFINE_RANGE("edge_place");
    hipLaunchKernelGGL(k_edge_place, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, g, edge_ids, t_lo, t_hi, s_lo, s_hi, level,
                       (long long)n, verts, counts);
    return check_launch("k_edge_place");
}

int mofa_fd_points(const float* verts, const float h[3], int64_t first, int64_t n, float* pts, void* stream) {
    const int rc = spacing_check(h, "fd_points");
    if (rc != MOFA_OK) return rc;
    MOFA_REQUIRE(verts && pts, "fd_points: null pointer");
    MOFA_REFINE_RANGE("fd_points");
    MOFA_REQUIRE(first >= 0 && first <= (1ll << 60), "fd_points: first = %lld", (long long)first);
    hipLaunchKernelGGL(k_fd_points, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, verts, h[0], h[1], h[2], (long long)first,
                       (long long)n, pts);
    return check_launch("k_fd_points");
}

int mofa_fd_normals(const float* s, const float h[3], int64_t n, float* normals, int64_t* counts, void* stream) {
    const int rc = spacing_check(h, "fd_normals");
    if (rc != MOFA_OK) return rc;
    MOFA_REQUIRE(s && normals && counts, "fd_normals: null pointer");
    MOFA_REFINE_RANGE("fd_normals");
    hipLaunchKernelGGL(k_fd_normals, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, s, h[0], h[1], h[2], (long long)n, normals, counts);
    return check_launch("k_fd_normals");
}

}  // extern "C"
