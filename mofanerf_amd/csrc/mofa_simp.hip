// Mesh simplification for the geometry export (gfx950): vertex clustering on a lattice of cells with one quadric-error representative per
// cluster (Rossignac-Borrel clustering, Lindstrom's placement).  mesh.py drives the passes (mesh.simplify); nothing here waits on another
// thread, no float or double atomic exists (the only atomics are the integer counters), and every kernel checks the indices it
// dereferences: a bad index is counted in counts[MOFA_SIMP_BAD_INDEX] and skipped, never a fault.
//
//   keys      per vertex, in fp32, every operation rounded separately:  q_a = floorf((x_a - origin_a) / cell_a),
//             key = (q_x << 42) | (q_y << 21) | q_z (int64).  A vertex with a non-finite coordinate or a q_a outside [0, 2^21) gets key -1
//             and is counted in counts[MOFA_SIMP_BAD_VERTEX].
//   quadrics  per face, in fp64 from the fp32 coordinates, every operation rounded separately:  u = v1 - v0, w = v2 - v0,
//             n = (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx), d = -((nx v0x + ny v0y) + nz v0z);
//             the row is  nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d  (A00 A01 A02 A11 A12 A22 b0 b1 b2 c).
//             The (cluster, quadric) pair of corner c of face f is pair 3 f + c; the pairs are NOT materialised: seg_sum reads row
//             perm[i] / row_div of the per-face rows (row_div = 3), 80 F bytes instead of 240 F.
//   seg_sum   out[s] = the sum of rows perm[i] / row_div, i in [seg_start[s], seg_end[s]), of in[N, NCOLS] (NCOLS = 4 or 10): one workgroup
//             per segment, thread t adds its rows i = s0 + t, s0 + t + 256, ... in that order starting from +0.0, then a fixed tree over the
//             256 partial sums (t < w: sm[t] += sm[t + w], w = 128, 64, ..., 1).  mofa_cc_seg_sum's scheme for NCOLS columns.
//   place     per cluster, in fp64, every operation rounded separately, in exactly this order:
//               m_a = S_a / S_3 (S = the cluster's sum of (x, y, z, 1));  w = regularize * ((A00 + A11) + A22)
//               a00 = A00 + w, a11 = A11 + w, a22 = A22 + w, a01 = A01, a02 = A02, a12 = A12;  r_a = w * m_a - b_a
//               c00 = a11 a22 - a12 a12,  c01 = a02 a12 - a01 a22,  c02 = a01 a12 - a02 a11,
//               c11 = a00 a22 - a02 a02,  c12 = a01 a02 - a00 a12,  c22 = a00 a11 - a01 a01
//               det = (a00 c00 + a01 c01) + a02 c02
//               x_0 = ((c00 r0 + c01 r1) + c02 r2) / det,  x_1 = ((c01 r0 + c11 r1) + c12 r2) / det,  x_2 = ((c02 r0 + c12 r1) + c22 r2) / det
//             x rounded to fp32 is the representative iff w > 0, w and det are finite, det > 0 and the keys arithmetic on the rounded point
//             gives the cluster's own key; otherwise m rounded to fp32 under the same key test; otherwise the cluster's first vertex.
//             mode = MOFA_SIMP_PLACE_MEAN starts at the mean.  counts[MOFA_SIMP_QUADRIC / _MEAN / _FIRST] count the route taken,
//             counts[MOFA_SIMP_MEAN_REQUESTED] the clusters that were asked to start at the mean.
//   faces     new[c] = cluster[faces[f][c]]; degenerate[f] = two of them are equal (or an index is bad); a surviving face is written in
//             its canonical rotation: the smallest index first, the cyclic order (the orientation) kept.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kSimpMaxIndex = (1ll << 31) - 1;     // V, F, C and every segment count: int32 indices; anything indexed by 3 F is 64-bit
constexpr float kSimpCells = 2097152.0f;                 // 2^21 cells per axis

__device__ __forceinline__ bool simp_in_range(int v, int V) { return (unsigned)v < (unsigned)V; }

// counts[slot] += the lanes of this wavefront for which pred holds: one integer atomic per wavefront and slot
__device__ __forceinline__ void simp_count(int64_t* counts, int slot, bool pred) {
    const unsigned long long b = __ballot(pred);
    if (pred && (int)__lane_id() == __ffsll(b) - 1) atomicAdd((unsigned long long*)(counts + slot), (unsigned long long)__popcll(b));
}

struct SimpGrid {
    float origin[3], cell[3];
};

// the cell key of a point, or -1: fp32, (x - origin) / cell with the correctly rounded division, floorf
__device__ __forceinline__ long long simp_key(const float (&p)[3], const SimpGrid& g) {
    long long key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = floorf(__fdiv_rn(__fsub_rn(p[a], g.origin[a]), g.cell[a]));
        if (!(t >= 0.0f && t < kSimpCells)) return -1;        // (NaN fails both comparisons)
        key = (key << 21) | (long long)(int)t;
    }
    return key;
}

__global__ __launch_bounds__(256) void k_simp_keys(const float* __restrict__ verts, int V, SimpGrid g, long long* __restrict__ keys,
                                                   int64_t* __restrict__ counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float p[3] = {verts[v * 3 + 0], verts[v * 3 + 1], verts[v * 3 + 2]};
    const long long key = simp_key(p, g);
    keys[v] = key;
    if (key < 0) atomicAdd((unsigned long long*)(counts + MOFA_SIMP_BAD_VERTEX), 1ull);
}

__global__ __launch_bounds__(256) void k_simp_quadrics(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V,
                                                       double* __restrict__ quadrics, int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    double* out = quadrics + f * 10;
    if (!simp_in_range(i0, V) || !simp_in_range(i1, V) || !simp_in_range(i2, V)) {
#pragma unroll
        for (int k = 0; k < 10; ++k) out[k] = 0.0;
        atomicAdd((unsigned long long*)(counts + MOFA_SIMP_BAD_INDEX), 1ull);
        return;
    }
    double p[3], q[3], r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (double)verts[(long long)i0 * 3 + c], q[c] = (double)verts[(long long)i1 * 3 + c], r[c] = (double)verts[(long long)i2 * 3 + c];
    const double ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
    const double wx = r[0] - p[0], wy = r[1] - p[1], wz = r[2] - p[2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double d = -((nx * p[0] + ny * p[1]) + nz * p[2]);
    out[0] = nx * nx, out[1] = nx * ny, out[2] = nx * nz, out[3] = ny * ny, out[4] = ny * nz, out[5] = nz * nz;
    out[6] = nx * d, out[7] = ny * d, out[8] = nz * d, out[9] = d * d;
}

// `iters` (from the host: ceil(longest segment / 256)) fixes the trip count; the segment's own ends only mask rows out
template <int NCOLS>
__global__ __launch_bounds__(256) void k_simp_seg_sum(const double* __restrict__ in, const int64_t* __restrict__ perm, int row_div, long long N,
                                                      const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end, int iters,
                                                      double* __restrict__ out) {
    __shared__ double sm[NCOLS][256];
    const long long s = blockIdx.x;
    const long long n_index = perm ? N * row_div : N;          // how many entries the segments index: perm's length, or the rows themselves
    long long s0 = seg_start[s], s1 = seg_end[s];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > n_index ? n_index : s1;
    const int t = threadIdx.x;
    double acc[NCOLS];
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) acc[c] = 0.0;
    for (int k = 0; k < iters; ++k) {
        const long long i = s0 + t + (long long)k * 256;
        if (i < s1) {
            long long row = perm ? perm[i] : i;
            if (row >= 0 && row < n_index) {
                row /= row_div;
#pragma unroll
                for (int c = 0; c < NCOLS; ++c) acc[c] += in[row * NCOLS + c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) sm[c][t] = acc[c];
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) sm[c][t] += sm[c][t + w];
        }
        __syncthreads();
    }
    if (t < NCOLS) out[s * NCOLS + t] = sm[t][0];
}

__global__ __launch_bounds__(256) void k_simp_place(const double* __restrict__ quadrics, const double* __restrict__ vsum,
                                                    const long long* __restrict__ cluster_keys, const int* __restrict__ first,
                                                    const float* __restrict__ verts, int V, int C, SimpGrid g, double regularize, int mode,
                                                    float* __restrict__ out, int64_t* __restrict__ counts) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const long long want = cluster_keys[c];
    const double* S = vsum + c * 4;
    const double m[3] = {S[0] / S[3], S[1] / S[3], S[2] / S[3]};
    float rep[3];
    int route = -1;
    if (mode != MOFA_SIMP_PLACE_MEAN) {
        const double* Q = quadrics + c * 10;
        const double w = regularize * ((Q[0] + Q[3]) + Q[5]);
        if (w > 0.0 && isfinite(w)) {
            const double a00 = Q[0] + w, a11 = Q[3] + w, a22 = Q[5] + w, a01 = Q[1], a02 = Q[2], a12 = Q[4];
            const double r0 = w * m[0] - Q[6], r1 = w * m[1] - Q[7], r2 = w * m[2] - Q[8];
            const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
            const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
            const double det = (a00 * c00 + a01 * c01) + a02 * c02;
            if (det > 0.0 && isfinite(det)) {
                const double x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
                const double x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
                const double x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
                rep[0] = (float)x0, rep[1] = (float)x1, rep[2] = (float)x2;
                if (want >= 0 && simp_key(rep, g) == want) route = MOFA_SIMP_QUADRIC;      // (a non-finite point has key -1)
            }
        }
    }
    if (route < 0) {
        rep[0] = (float)m[0], rep[1] = (float)m[1], rep[2] = (float)m[2];
        if (want >= 0 && simp_key(rep, g) == want) route = MOFA_SIMP_MEAN;
    }
    if (route < 0) {
        const int v = first[c];
        if (simp_in_range(v, V)) {
            rep[0] = verts[(long long)v * 3 + 0], rep[1] = verts[(long long)v * 3 + 1], rep[2] = verts[(long long)v * 3 + 2];
        } else {
            rep[0] = rep[1] = rep[2] = 0.0f;
            atomicAdd((unsigned long long*)(counts + MOFA_SIMP_BAD_INDEX), 1ull);
        }
        route = MOFA_SIMP_FIRST;
    }
    out[c * 3 + 0] = rep[0], out[c * 3 + 1] = rep[1], out[c * 3 + 2] = rep[2];
    simp_count(counts, MOFA_SIMP_QUADRIC, route == MOFA_SIMP_QUADRIC);
    simp_count(counts, MOFA_SIMP_MEAN, route == MOFA_SIMP_MEAN);
    simp_count(counts, MOFA_SIMP_FIRST, route == MOFA_SIMP_FIRST);
    simp_count(counts, MOFA_SIMP_MEAN_REQUESTED, mode == MOFA_SIMP_PLACE_MEAN);
}

__global__ __launch_bounds__(256) void k_simp_faces(const int* __restrict__ faces, long long F, int V, const int* __restrict__ cluster, int C,
                                                    int* __restrict__ out, unsigned char* __restrict__ degenerate, int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int n[3];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = faces[f * 3 + c];
        n[c] = simp_in_range(v, V) ? cluster[v] : -1;
        bad |= !simp_in_range(n[c], C);
    }
    if (bad) {
        atomicAdd((unsigned long long*)(counts + MOFA_SIMP_BAD_INDEX), 1ull);
        out[f * 3 + 0] = out[f * 3 + 1] = out[f * 3 + 2] = -1;
        degenerate[f] = 1;
        return;
    }
    degenerate[f] = n[0] == n[1] || n[1] == n[2] || n[2] == n[0];
    const int k = (n[1] < n[0] && n[1] <= n[2]) ? 1 : ((n[2] < n[0] && n[2] < n[1]) ? 2 : 0);     // the first smallest
    out[f * 3 + 0] = n[k], out[f * 3 + 1] = n[(k + 1) % 3], out[f * 3 + 2] = n[(k + 2) % 3];
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

bool simp_grid(const float* origin, const float* cell, SimpGrid& g) {
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = origin[a], g.cell[a] = cell[a];
        if (!isfinite(origin[a]) || !isfinite(cell[a]) || !(cell[a] > 0.0f)) return false;
    }
    return true;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_SIMP_COUNT(what, name, n) \
    MOFA_REQUIRE((n) >= 1 && (n) <= kSimpMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

extern "C" {

int mofa_simp_keys(const float* verts, int64_t V, const float origin[3], const float cell[3], int64_t* keys, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts && origin && cell && keys && counts, "simp_keys: null pointer");
    MOFA_SIMP_COUNT("simp_keys", "V", V);
    SimpGrid g;
    MOFA_REQUIRE(simp_grid(origin, cell, g), "simp_keys: origin / cell must be finite and cell > 0");
    hipLaunchKernelGGL(k_simp_keys, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, verts, (int)V, g, (long long*)keys, counts);
    return check_launch("k_simp_keys");
}

int mofa_simp_corner_quadrics(const float* verts, const int32_t* faces, int64_t F, int64_t V, double* quadrics, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts && faces && quadrics && counts, "simp_corner_quadrics: null pointer");
    MOFA_SIMP_COUNT("simp_corner_quadrics", "F", F);
    MOFA_SIMP_COUNT("simp_corner_quadrics", "V", V);
    hipLaunchKernelGGL(k_simp_quadrics, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, quadrics, counts);
    return check_launch("k_simp_quadrics");
}

int mofa_simp_seg_sum(const double* in, int32_t ncols, const int64_t* perm, int32_t row_div, int64_t N, const int64_t* seg_start,
                      const int64_t* seg_end, int64_t n_segments, int64_t longest, double* out, void* stream) {
    MOFA_REQUIRE(in && seg_start && seg_end && out, "simp_seg_sum: null pointer");
    MOFA_REQUIRE(ncols == 4 || ncols == 10, "simp_seg_sum: ncols = %d (want 4 or 10)", (int)ncols);
    MOFA_REQUIRE(row_div >= 1 && row_div <= 3 && (perm || row_div == 1), "simp_seg_sum: row_div = %d (want 1 .. 3, and 1 without perm)", (int)row_div);
    MOFA_SIMP_COUNT("simp_seg_sum", "N", N);
    MOFA_SIMP_COUNT("simp_seg_sum", "n_segments", n_segments);
    MOFA_REQUIRE(longest >= 0 && longest <= 3 * kSimpMaxIndex, "simp_seg_sum: longest = %lld (want 0 .. 3 (2^31 - 1))", (long long)longest);
    const int iters = (int)((longest + 255) / 256);
    if (ncols == 4)
        hipLaunchKernelGGL(k_simp_seg_sum<4>, dim3((unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, in, perm, (int)row_div, (long long)N,
                           seg_start, seg_end, iters, out);
    else
        hipLaunchKernelGGL(k_simp_seg_sum<10>, dim3((unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, in, perm, (int)row_div, (long long)N,
                           seg_start, seg_end, iters, out);
    return check_launch("k_simp_seg_sum");
}

int mofa_simp_place(const double* quadrics, const double* vsum, const int64_t* cluster_keys, const int32_t* first, const float* verts, int64_t V,
                    int64_t C, const float origin[3], const float cell[3], double regularize, int32_t mode, float* out, int64_t* counts,
                    void* stream) {
    MOFA_REQUIRE(vsum && cluster_keys && first && verts && origin && cell && out && counts, "simp_place: null pointer");
    MOFA_REQUIRE(mode == MOFA_SIMP_PLACE_QUADRIC || mode == MOFA_SIMP_PLACE_MEAN, "simp_place: mode = %d", (int)mode);
    MOFA_REQUIRE(quadrics || mode == MOFA_SIMP_PLACE_MEAN, "simp_place: the quadric placement needs the quadrics");
    MOFA_REQUIRE(isfinite(regularize) && regularize > 0.0, "simp_place: regularize = %g (want finite and > 0)", regularize);
    MOFA_SIMP_COUNT("simp_place", "V", V);
    MOFA_SIMP_COUNT("simp_place", "C", C);
    SimpGrid g;
    MOFA_REQUIRE(simp_grid(origin, cell, g), "simp_place: origin / cell must be finite and cell > 0");
    hipLaunchKernelGGL(k_simp_place, dim3(blocks_of(C)), dim3(256), 0, (hipStream_t)stream, quadrics, vsum, (const long long*)cluster_keys, first,
                       verts, (int)V, (int)C, g, regularize, (int)mode, out, counts);
    return check_launch("k_simp_place");
}

int mofa_simp_faces(const int32_t* faces, int64_t F, int64_t V, const int32_t* cluster, int64_t C, int32_t* out, uint8_t* degenerate,
                    int64_t* counts, void* stream) {
    MOFA_REQUIRE(faces && cluster && out && degenerate && counts, "simp_faces: null pointer");
    MOFA_SIMP_COUNT("simp_faces", "F", F);
    MOFA_SIMP_COUNT("simp_faces", "V", V);
    MOFA_SIMP_COUNT("simp_faces", "C", C);
    hipLaunchKernelGGL(k_simp_faces, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, faces, (long long)F, (int)V, cluster, (int)C, out,
                       degenerate, counts);
    return check_launch("k_simp_faces");
}

}  // extern "C"
