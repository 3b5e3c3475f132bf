// Mesh smoothing for the geometry export (gfx950): Taubin lambda | mu filtering on a fixed-order vertex adjacency.  mesh.py drives the
// passes (mesh.smooth): it builds the adjacency (sorted directed pairs), launches the weights once and one step per pass, ping-ponging two
// vertex buffers.  Nothing here waits on another thread, no float or double atomic exists (the only atomics are the integer counters), and
// every kernel checks the indices it dereferences: a bad index is counted in counts[MOFA_SMOOTH_BAD_INDEX] and skipped, never a fault.
// All arithmetic is fp64 on the fp32 coordinates widened, every operation rounded separately (the build pins -ffp-contract=off).
//
//   corner_cots   for face f and corner c with apex o = f[c], a = f[(c + 1) % 3], b = f[(c + 2) % 3]:
//                   u = x_a - x_o, v = x_b - x_o;  cr = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx);  n = sqrt((crx crx + cry cry) + crz crz)
//                   cots[3 f + c] = ((ux vx + uy vy) + uz vz) / n;  n == 0 or not finite: 0, counted in counts[MOFA_SMOOTH_FLAT_CORNERS]
//   edge_weights  half-edge entry e = 2 (3 f + c) + dir carries the directed pair (a, b) for dir = 0 and (b, a) for dir = 1; the host sorts
//                 the entries stably by (i << 31) | j (perm) and gives the runs of the E distinct pairs (seg).  One thread per pair:
//                   w = 0.0;  for k in [seg[p], seg[p + 1]): w += 0.5 * cots[perm[k] / 2];  w < 0: w = 0, counted in
//                   counts[MOFA_SMOOTH_NEGATIVE_WEIGHTS].  (i, j) and (j, i) run over the same corners in the same order: w_ij == w_ji.
//   step          one thread per vertex i, its neighbours nbr[offsets[i] .. offsets[i + 1]) in list order (ascending index), per component:
//                   uniform:   s = 0.0;  s += (double)x_j - (double)x_i;  L = s / (double)deg
//                   weighted:  s = 0.0, sw = 0.0;  s += w_ij * ((double)x_j - (double)x_i), sw += w_ij;  L = s / sw  (needs sw > 0; otherwise
//                              the vertex keeps its bits and is counted in counts[MOFA_SMOOTH_ZERO_WEIGHT])
//                   out = (float)((double)x_i + factor * L)
//                 A pinned vertex and one without neighbours keep their bits.  A vertex with a neighbour outside [0, V), or whose list does
//                 not lie in [0, E), writes nothing and is counted.  in and out are different buffers.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kSmoothMaxIndex = (1ll << 31) - 1;     // V, F, E: int32 indices, one thread per element; 6 F entries are 64-bit

__device__ __forceinline__ bool smooth_in_range(int v, int V) { return (unsigned)v < (unsigned)V; }

__global__ __launch_bounds__(256) void k_smooth_corner_cots(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V,
                                                            double* __restrict__ cots, int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int idx[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
    if (!smooth_in_range(idx[0], V) || !smooth_in_range(idx[1], V) || !smooth_in_range(idx[2], V)) {
        cots[f * 3 + 0] = 0.0, cots[f * 3 + 1] = 0.0, cots[f * 3 + 2] = 0.0;
        atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_BAD_INDEX), 1ull);
        return;
    }
    double x[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) x[c][k] = (double)verts[(long long)idx[c] * 3 + k];
    int flat = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double(&o)[3] = x[c];
        const double(&a)[3] = x[(c + 1) % 3];
        const double(&b)[3] = x[(c + 2) % 3];
        const double ux = a[0] - o[0], uy = a[1] - o[1], uz = a[2] - o[2];
        const double vx = b[0] - o[0], vy = b[1] - o[1], vz = b[2] - o[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double n = sqrt((cx * cx + cy * cy) + cz * cz);
        const double d = (ux * vx + uy * vy) + uz * vz;
        const bool ok = n != 0.0 && isfinite(n);
        cots[f * 3 + c] = ok ? d / n : 0.0;
        flat += !ok;
    }
    if (flat) atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_FLAT_CORNERS), (unsigned long long)flat);
}

__global__ __launch_bounds__(256) void k_smooth_edge_weights(const double* __restrict__ cots, long long n_cots, const int64_t* __restrict__ perm,
                                                             long long P, const int64_t* __restrict__ seg, long long E,
                                                             double* __restrict__ weights, int64_t* __restrict__ counts) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const long long k0 = seg[p], k1 = seg[p + 1];
    if (k0 < 0 || k1 < k0 || k1 > P) {
        weights[p] = 0.0;
        atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_BAD_INDEX), 1ull);
        return;
    }
    double w = 0.0;
    int bad = 0;
    for (long long k = k0; k < k1; ++k) {
        const long long e = perm[k];
        if (e < 0 || (e >> 1) >= n_cots) {
            ++bad;
            continue;
        }
        w += 0.5 * cots[e >> 1];
    }
    if (bad) atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_BAD_INDEX), (unsigned long long)bad);
    if (w < 0.0) {
        w = 0.0;
        atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_NEGATIVE_WEIGHTS), 1ull);
    }
    weights[p] = w;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_smooth_step(const float* __restrict__ in, int V, const int64_t* __restrict__ offsets,
                                                     const int* __restrict__ nbr, long long E, const double* __restrict__ weights,
                                                     const uint8_t* __restrict__ pinned, double factor, float* __restrict__ out,
                                                     int64_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float xi[3] = {in[i * 3 + 0], in[i * 3 + 1], in[i * 3 + 2]};
    const long long k0 = offsets[i], k1 = offsets[i + 1];
    if (k0 < 0 || k1 < k0 || k1 > E) {
        atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_BAD_INDEX), 1ull);
        return;
    }
    if ((pinned && pinned[i]) || k1 == k0) {
        out[i * 3 + 0] = xi[0], out[i * 3 + 1] = xi[1], out[i * 3 + 2] = xi[2];
        return;
    }
    const double px = (double)xi[0], py = (double)xi[1], pz = (double)xi[2];
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    for (long long k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (!smooth_in_range(j, V)) {
            atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_BAD_INDEX), 1ull);
            return;
        }
        const double dx = (double)in[(long long)j * 3 + 0] - px, dy = (double)in[(long long)j * 3 + 1] - py,
                     dz = (double)in[(long long)j * 3 + 2] - pz;
        if (WEIGHTED) {
            const double w = weights[k];
            sx += w * dx, sy += w * dy, sz += w * dz;
            sw += w;
        } else {
            sx += dx, sy += dy, sz += dz;
        }
    }
    if (!WEIGHTED) sw = (double)(k1 - k0);
    if (WEIGHTED && !(sw > 0.0)) {
        out[i * 3 + 0] = xi[0], out[i * 3 + 1] = xi[1], out[i * 3 + 2] = xi[2];
        atomicAdd((unsigned long long*)(counts + MOFA_SMOOTH_ZERO_WEIGHT), 1ull);
        return;
    }
    out[i * 3 + 0] = (float)(px + factor * (sx / sw));
    out[i * 3 + 1] = (float)(py + factor * (sy / sw));
    out[i * 3 + 2] = (float)(pz + factor * (sz / sw));
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_SMOOTH_COUNT(what, name, n) \
    MOFA_REQUIRE((n) >= 1 && (n) <= kSmoothMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

extern "C" {

int mofa_smooth_corner_cots(const float* verts, const int32_t* faces, int64_t F, int64_t V, double* cots, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts && faces && cots && counts, "smooth_corner_cots: null pointer");
    MOFA_SMOOTH_COUNT("smooth_corner_cots", "F", F);
    MOFA_SMOOTH_COUNT("smooth_corner_cots", "V", V);
    hipLaunchKernelGGL(k_smooth_corner_cots, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, cots,
                       counts);
    return check_launch("k_smooth_corner_cots");
}

int mofa_smooth_edge_weights(const double* cots, int64_t F, const int64_t* perm, int64_t P, const int64_t* seg, int64_t E, double* weights,
                             int64_t* counts, void* stream) {
    MOFA_REQUIRE(cots && perm && seg && weights && counts, "smooth_edge_weights: null pointer");
    MOFA_SMOOTH_COUNT("smooth_edge_weights", "F", F);
    MOFA_SMOOTH_COUNT("smooth_edge_weights", "E", E);
    MOFA_REQUIRE(P >= E && P <= 6 * F, "smooth_edge_weights: P = %lld entries for E = %lld pairs of F = %lld faces (want E .. 6 F)", (long long)P,
                 (long long)E, (long long)F);
    hipLaunchKernelGGL(k_smooth_edge_weights, dim3(blocks_of(E)), dim3(256), 0, (hipStream_t)stream, cots, 3 * (long long)F, perm, (long long)P,
                       seg, (long long)E, weights, counts);
    return check_launch("k_smooth_edge_weights");
}

int mofa_smooth_step(const float* verts_in, int64_t V, const int64_t* offsets, const int32_t* nbr, int64_t E, const double* weights,
                     const uint8_t* pinned, double factor, float* verts_out, int64_t* counts, void* stream) {
    MOFA_REQUIRE(verts_in && offsets && nbr && verts_out && counts, "smooth_step: null pointer");
    MOFA_REQUIRE(verts_in != verts_out, "smooth_step: the step does not run in place (verts_in == verts_out)");
    MOFA_SMOOTH_COUNT("smooth_step", "V", V);
    MOFA_SMOOTH_COUNT("smooth_step", "E", E);
    MOFA_REQUIRE(isfinite(factor), "smooth_step: factor = %g (want finite)", factor);
    if (weights)
        hipLaunchKernelGGL(k_smooth_step<true>, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, verts_in, (int)V, offsets, nbr, (long long)E,
                           weights, pinned, factor, verts_out, counts);
    else
        hipLaunchKernelGGL(k_smooth_step<false>, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, verts_in, (int)V, offsets, nbr,
                           (long long)E, weights, pinned, factor, verts_out, counts);
    return check_launch("k_smooth_step");
}

}  // extern "C"
