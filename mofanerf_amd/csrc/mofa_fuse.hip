// Depth-map fusion for the geometry export (gfx950): a truncated signed distance volume on the lattice of mofa_grid_points, integrated from
// depth frames view by view, and the marchable field made from it.  mesh.py drives the passes (mesh.tsdf_volume / tsdf_integrate / tsdf_field /
// tsdf_surface).  One thread per voxel; a voxel's four state values are read once, updated over the views of the call IN ORDER and written
// once: no atomics, nothing waits on another thread, the same frames in the same order give the same bytes, and views [a | b] in two calls
// give the bytes of one call with a + b.  All arithmetic is fp64 on the fp32 inputs widened, every operation rounded separately (the build
// pins -ffp-contract=off).  The camera of a view (fx, fy, cx, cy and the 3 x 4 pose: 16 floats) is read with a wave-uniform index, so it
// travels in scalar registers; the depth (and weight) samples are the only gathers, and every index is range-checked before it is used.
//
//   integrate   voxel idx = (i ny + j) nz + k at x = (lo_x + (float)i step_x, ..) (the bits of mofa_grid_points); per view, c = its pose:
//                 d[a] = x[a] - c[a][3];  p[a] = (d0 c[0][a] + d1 c[1][a]) + d2 c[2][a]   (the rotation transposed: the pose is ASSUMED
//                 orthonormal, as in mofa_raster_project);  t = -p[2]: the ray parameter of get_rays, whose direction has camera z = -1
//                 not t > 0: the view does not see the voxel
//                 u = cx + fx (p0 / t), v = cy - fy (p1 / t);  pu = floor(u + 0.5), pv = floor(v + 0.5);  0 <= pu < W and 0 <= pv < H
//                 tested on the doubles (a non-finite value fails), otherwise the view does not see the voxel
//                 D = depth[view][pv][pu]:  not D > 0 (NaN, -inf, 0, negative): unknown, skip;  D = +inf: background, s = 1 when carve, skip
//                 otherwise;  else sdf = D - t;  sdf < -trunc: behind += 1, skip;  s = sdf / trunc, s > 1: s = 1
//                 w = weight[view][pv][pu] (1 without a map);  w == 0: skip;  acc = acc + w s, wsum = wsum + w, front += 1
//   field       wsum > 0: field = (float)(-(acc / wsum));  otherwise +1 or -1 by `unobserved`;  close_border: the outermost layer = -1
#include <math.h>

#include "mofa_lattice.h"

namespace mofa {
namespace {

constexpr long long kFuseMaxIndex = (1ll << 31) - 1;     // voxels of a volume, pixels of a frame: one thread / one int32 index each

__global__ __launch_bounds__(256) void k_tsdf_integrate(long long n, int ny, int nz, float lox, float loy, float loz, float sx, float sy, float sz,
                                                        double trunc, const float* __restrict__ depth, const float* __restrict__ weight,
                                                        int n_views, int H, int W, const float* __restrict__ cams, int per_view_cam, int carve,
                                                        double* __restrict__ acc, double* __restrict__ wsum, int* __restrict__ front,
                                                        int* __restrict__ behind) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const long long plane = (long long)ny * nz;
    const long long i = idx / plane, r = idx - i * plane, j = r / nz, k = r - j * nz;
    const double x0 = (double)grid_coord(lox, sx, i), x1 = (double)grid_coord(loy, sy, j), x2 = (double)grid_coord(loz, sz, k);
    double a = acc[idx], ws = wsum[idx];
    int nf = front[idx], nb = behind[idx];
    const long long frame = (long long)H * W;
    for (int view = 0; view < n_views; ++view) {
        const float* __restrict__ c = cams + (per_view_cam ? (long long)view * 16 : 0);     // wave-uniform: scalar loads
        const double fx = (double)c[0], fy = (double)c[1], cx = (double)c[2], cy = (double)c[3];
        const float* __restrict__ m = c + 4;                                                // pose [3][4], row-major
        const double d0 = x0 - (double)m[3], d1 = x1 - (double)m[7], d2 = x2 - (double)m[11];
        const double p0 = (d0 * (double)m[0] + d1 * (double)m[4]) + d2 * (double)m[8];
        const double p1 = (d0 * (double)m[1] + d1 * (double)m[5]) + d2 * (double)m[9];
        const double p2 = (d0 * (double)m[2] + d1 * (double)m[6]) + d2 * (double)m[10];
        const double t = -p2;
        if (!(t > 0.0)) continue;
        const double u = cx + fx * (p0 / t), v = cy - fy * (p1 / t);
        const double pu = floor(u + 0.5), pv = floor(v + 0.5);
        if (!(pu >= 0.0 && pu < (double)W && pv >= 0.0 && pv < (double)H)) continue;
        const long long pix = (long long)view * frame + (long long)pv * W + (long long)pu;
        const float D = depth[pix];
        if (!(D > 0.0f)) continue;                       // NaN, -inf, 0, negative: unknown
        double s;
        if (D == INFINITY) {                             // background: the space along the ray is empty
            if (!carve) continue;
            s = 1.0;
        } else {
            const double sdf = (double)D - t;
            if (sdf < -trunc) {
                ++nb;
                continue;
            }
            s = sdf / trunc;
            if (s > 1.0) s = 1.0;
        }
        const double w = weight ? (double)weight[pix] : 1.0;
        if (w == 0.0) continue;
        a = a + w * s;
        ws = ws + w;
        ++nf;
    }
    acc[idx] = a, wsum[idx] = ws, front[idx] = nf, behind[idx] = nb;
}

// field + the four classes of this block's voxels (observed, filled inside, filled outside, border) to partial[block][4]
__global__ __launch_bounds__(256) void k_tsdf_field(long long n, int nx, int ny, int nz, const double* __restrict__ acc,
                                                    const double* __restrict__ wsum, const int* __restrict__ behind, int unobserved,
                                                    int close_border, float* __restrict__ field, int* __restrict__ partial) {
    __shared__ int s_counts[4][4];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    int mine[4] = {0, 0, 0, 0};
    if (idx < n) {
        const double ws = wsum[idx];
        float f;
        if (ws > 0.0) {
            f = (float)(-(acc[idx] / ws));
            mine[MOFA_TSDF_OBSERVED] = 1;
        } else {
            const bool in = unobserved == MOFA_TSDF_UNOBSERVED_INSIDE || (unobserved == MOFA_TSDF_UNOBSERVED_AUTO && behind[idx] > 0);
            f = in ? 1.0f : -1.0f;
            mine[MOFA_TSDF_FILLED_INSIDE] = in, mine[MOFA_TSDF_FILLED_OUTSIDE] = !in;
        }
        if (close_border) {
            const long long plane = (long long)ny * nz;
            const long long i = idx / plane, r = idx - i * plane, j = r / nz, k = r - j * nz;
            if (i == 0 || i == nx - 1 || j == 0 || j == ny - 1 || k == 0 || k == nz - 1) {
                f = -1.0f;
                mine[MOFA_TSDF_BORDER] = 1;
            }
        }
        field[idx] = f;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int v = mine[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_counts[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        partial[(long long)blockIdx.x * 4 + threadIdx.x] =
            ((s_counts[0][threadIdx.x] + s_counts[1][threadIdx.x]) + s_counts[2][threadIdx.x]) + s_counts[3][threadIdx.x];
}

// counts[q] = the sum of partial[b][q] over the blocks, in a fixed order: thread t takes b = t, t + 256, .., then a tree over the threads
__global__ __launch_bounds__(256) void k_tsdf_counts(const int* __restrict__ partial, long long blocks, int64_t* __restrict__ counts) {
    __shared__ long long s[256][4];
    long long mine[4] = {0, 0, 0, 0};
    for (long long b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) mine[q] += partial[b * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[threadIdx.x][q] = mine[q];
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[threadIdx.x][q] += s[threadIdx.x + half][q];
        __syncthreads();
    }
    if (threadIdx.x < 4) counts[threadIdx.x] = s[0][threadIdx.x];
}

inline long long blocks_of(long long n) { return (n + 255) / 256; }

inline bool fuse_grid_ok(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > kFuseMaxIndex || ny > kFuseMaxIndex || nz > kFuseMaxIndex) return false;
    return nx * ny <= kFuseMaxIndex && nx * ny * nz <= kFuseMaxIndex;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_FUSE_GRID(what)                                                                                                       \
    MOFA_REQUIRE(fuse_grid_ok(nx, ny, nz), what ": grid %lld x %lld x %lld (want >= 2 samples per axis and nx ny nz < 2^31)", (long long)nx, \
                 (long long)ny, (long long)nz)

extern "C" {

size_t mofa_tsdf_state_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (!fuse_grid_ok(nx, ny, nz)) return 0;
    return (size_t)(nx * ny * nz) * 24;
}

size_t mofa_tsdf_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (!fuse_grid_ok(nx, ny, nz)) return 0;
    return (size_t)blocks_of(nx * ny * nz) * 4 * sizeof(int);
}

int mofa_tsdf_integrate(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], double trunc, const float* depth,
                        const float* weight, int64_t n_views, int32_t H, int32_t W, const float* cams, int64_t n_cams, int32_t carve, double* acc,
                        double* wsum, int32_t* front, int32_t* behind, void* stream) {
    MOFA_REQUIRE(lo && step && depth && cams && acc && wsum && front && behind, "tsdf_integrate: null pointer");
    MOFA_FUSE_GRID("tsdf_integrate");
    MOFA_REQUIRE(isfinite(trunc) && trunc > 0.0, "tsdf_integrate: trunc = %g (want finite and > 0)", trunc);
    MOFA_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= kFuseMaxIndex, "tsdf_integrate: H = %d, W = %d (want H, W >= 1 and H W < 2^31)", (int)H,
                 (int)W);
    MOFA_REQUIRE(n_views >= 1 && n_views <= kFuseMaxIndex, "tsdf_integrate: n_views = %lld (want 1 .. 2^31 - 1)", (long long)n_views);
    MOFA_REQUIRE(n_cams == 1 || n_cams == n_views, "tsdf_integrate: %lld cameras for %lld views (want 1 or one per view)", (long long)n_cams,
                 (long long)n_views);
    const long long n = nx * ny * nz;
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)blocks_of(n)), dim3(256), 0, (hipStream_t)stream, n, (int)ny, (int)nz, lo[0], lo[1], lo[2],
                       step[0], step[1], step[2], trunc, depth, weight, (int)n_views, (int)H, (int)W, cams, (int)(n_cams != 1), (int)(carve != 0), acc,
                       wsum, front, behind);
    return check_launch("k_tsdf_integrate");
}

int mofa_tsdf_field(int64_t nx, int64_t ny, int64_t nz, const double* acc, const double* wsum, const int32_t* behind, int32_t unobserved,
                    int32_t close_border, float* field, void* workspace, int64_t* counts, void* stream) {
    MOFA_REQUIRE(acc && wsum && behind && field && workspace && counts, "tsdf_field: null pointer");
    MOFA_FUSE_GRID("tsdf_field");
    MOFA_REQUIRE(unobserved == MOFA_TSDF_UNOBSERVED_AUTO || unobserved == MOFA_TSDF_UNOBSERVED_OUTSIDE || unobserved == MOFA_TSDF_UNOBSERVED_INSIDE,
                 "tsdf_field: unobserved = %d (want MOFA_TSDF_UNOBSERVED_AUTO, _OUTSIDE or _INSIDE)", (int)unobserved);
    const long long n = nx * ny * nz, blocks = blocks_of(n);
    hipLaunchKernelGGL(k_tsdf_field, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, (int)nx, (int)ny, (int)nz, acc, wsum, behind,
                       (int)unobserved, (int)(close_border != 0), field, (int*)workspace);
    if (int rc = check_launch("k_tsdf_field")) return rc;
    hipLaunchKernelGGL(k_tsdf_counts, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)workspace, blocks, counts);
    return check_launch("k_tsdf_counts");
}

}  // extern "C"
