// Mesh rasteriser (gfx950): depth, face index, barycentrics, attributes and flat normals of a triangle mesh in the camera convention of
// pinhole_ray / k_get_rays — pixel (i, j) is sampled at the integer point (i, j), the camera looks along -z, and the depth is the ray
// parameter of that pixel's ray, the quantity mofa_composite_sigma / mofa_depth_median give per ray.  DESIGN.md 3.13.
//
//   project   one lane per vertex: d = v - t, p_a = (d0 c[0][a] + d1 c[1][a]) + d2 c[2][a], zc = -p_2, u = cx + fx (p_0 / zc),
//             v = cy - fy (p_1 / zc) in separately rounded fp32; valid iff zc >= znear, |u| <= 2^20, |v| <= 2^20 (false for NaN);
//             X = rint(256 u), Y = rint(256 v): 1/256-pixel fixed point
//   coverage  int64 edge functions of the snapped vertices at P = (256 i, 256 j), all three >= 0 after multiplying by sign(A): both
//             windings are drawn, a sample on a shared edge belongs to both triangles
//   depth     fp64: l_k = w_k / |A|, q = (l0/z0 + l1/z1) + l2/z2, depth = (float)(1 / q) — ONE rounding to fp32
//   z-buffer  uint64 per pixel, all ones when empty, 64-bit atomicMin of (depth bits << 32) | face: depth > 0, so its bits order like
//             the value, and an equal depth falls to the lower face index.  The key is a pure function of (pixel, face): the frame does
//             not depend on the order of the atomics, and the resolve pass recomputes the winner's weights from the same integers.
//
// Two ways to walk a face behind that one z-buffer: a face whose clipped box holds fewer than wave_min_pixels pixels is walked by the
// lane that set it up (marching-tetrahedra meshes: most faces cover 0-2 samples); the others are appended to a list and walked one
// wavefront per face by a second kernel with a fixed grid, which reads the list's length from device memory.
//
// Kernels: k_raster_project, k_raster_clear, k_raster_setup, k_raster_wave, k_raster_resolve.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kRasterMax = 1ll << 31;       // pixels, vertices and faces: each fewer than this
constexpr float kGuardBand = 1048576.0f;          // 2^20 px: |X|, |Y| <= 2^28, edge products < 2^59
constexpr int kWaveBlocks = 1024;                 // k_raster_wave's fixed grid: 4096 wavefronts striding over the list
constexpr unsigned long long kEmpty = ~0ull;

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }
inline size_t align_up(size_t v) { return (v + 255) / 256 * 256; }

struct ProjVert {      // 16 B: one load per corner
    int X, Y;          // snapped screen position, 1/256 px
    float z;           // camera depth
    int valid;
};

struct RasterWs {
    unsigned* list_count;            // [0]: faces on the wave list
    unsigned long long* zbuf;        // [H W]
    ProjVert* pv;                    // [n_verts]
    int* list;                       // [n_faces]
    size_t bytes;
};

bool raster_sizes_ok(long long n_verts, long long n_faces, long long H, long long W) {
    return H >= 1 && W >= 1 && H * W < kRasterMax && n_verts >= 0 && n_faces >= 0 && n_verts < kRasterMax && n_faces < kRasterMax;
}

RasterWs raster_ws(void* base, long long n_verts, long long n_faces, long long H, long long W) {
    RasterWs w;
    char* p = (char*)base;
    size_t off = 0;
    w.list_count = (unsigned*)(p + off), off += 256;
    w.zbuf = (unsigned long long*)(p + off), off += align_up((size_t)(H * W) * sizeof(unsigned long long));
    w.pv = (ProjVert*)(p + off), off += align_up((size_t)n_verts * sizeof(ProjVert));
    w.list = (int*)(p + off), off += align_up((size_t)n_faces * sizeof(int));
    w.bytes = off;
    return w;
}

__global__ __launch_bounds__(256) void k_raster_project(const float* __restrict__ verts, long long n_verts, const float* __restrict__ c2w,
                                                        float fx, float fy, float cx, float cy, float znear, ProjVert* __restrict__ pv) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const float d0 = __fsub_rn(verts[v * 3 + 0], c2w[3]), d1 = __fsub_rn(verts[v * 3 + 1], c2w[7]), d2 = __fsub_rn(verts[v * 3 + 2], c2w[11]);
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        p[a] = __fadd_rn(__fadd_rn(__fmul_rn(d0, c2w[a]), __fmul_rn(d1, c2w[4 + a])), __fmul_rn(d2, c2w[8 + a]));
    const float zc = -p[2];
    const float u = __fadd_rn(cx, __fmul_rn(fx, __fdiv_rn(p[0], zc)));
    const float w = __fsub_rn(cy, __fmul_rn(fy, __fdiv_rn(p[1], zc)));
    const bool ok = zc >= znear && fabsf(u) <= kGuardBand && fabsf(w) <= kGuardBand;       // every comparison is false for NaN
    ProjVert o;
    o.X = ok ? (int)rintf(__fmul_rn(u, 256.0f)) : 0;
    o.Y = ok ? (int)rintf(__fmul_rn(w, 256.0f)) : 0;
    o.z = zc;
    o.valid = ok ? 1 : 0;
    pv[v] = o;
}

__global__ __launch_bounds__(256) void k_raster_clear(unsigned long long* __restrict__ zbuf, long long n_pixels, unsigned* __restrict__ list_count,
                                                      unsigned long long* __restrict__ counts) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < n_pixels) zbuf[p] = kEmpty;
    if (p < 4) counts[p] = 0;
    if (p == 0) list_count[0] = 0;
}

// A face ready to be walked: snapped corners, their depths, the sign of its doubled area and the box of samples clipped to the image.
struct Tri {
    long long X[3], Y[3];
    double z[3];
    long long s;          // sign(A)
    double area;          // (double)|A|
    long long i0, i1, j0, j1, npix;
};

enum { kFaceDrawn = 0, kFaceCulled = 1, kFaceDegenerate = 2 };

__device__ __forceinline__ int tri_setup(const int* __restrict__ faces, long long f, long long n_verts, const ProjVert* __restrict__ pv, int H, int W,
                                         Tri& t) {
    ProjVert c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int idx = faces[f * 3 + k];
        if (idx < 0 || idx >= n_verts) return kFaceCulled;
        c[k] = pv[idx];
    }
    if (!(c[0].valid && c[1].valid && c[2].valid)) return kFaceCulled;
#pragma unroll
    for (int k = 0; k < 3; ++k) t.X[k] = c[k].X, t.Y[k] = c[k].Y, t.z[k] = (double)c[k].z;
    const long long A = (t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
    if (A == 0) return kFaceDegenerate;
    t.s = A > 0 ? 1 : -1;
    t.area = (double)(A > 0 ? A : -A);
    const long long x0 = min(t.X[0], min(t.X[1], t.X[2])), x1 = max(t.X[0], max(t.X[1], t.X[2]));
    const long long y0 = min(t.Y[0], min(t.Y[1], t.Y[2])), y1 = max(t.Y[0], max(t.Y[1], t.Y[2]));
    t.i0 = max((x0 + 255) >> 8, 0ll), t.i1 = min(x1 >> 8, (long long)W - 1);       // ceil(min / 256) .. floor(max / 256), clipped
    t.j0 = max((y0 + 255) >> 8, 0ll), t.j1 = min(y1 >> 8, (long long)H - 1);
    t.npix = (t.i1 >= t.i0 && t.j1 >= t.j0) ? (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) : 0;
    return kFaceDrawn;
}

// w[k] = s E(k+1, k+2) at the sample (i, j); covered iff all three are >= 0
__device__ __forceinline__ bool tri_weights(const Tri& t, long long i, long long j, long long (&w)[3]) {
    const long long Px = i * 256, Py = j * 256;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = (k + 1) % 3, q = (k + 2) % 3;
        w[k] = t.s * ((t.X[q] - t.X[p]) * (Py - t.Y[p]) - (t.Y[q] - t.Y[p]) * (Px - t.X[p]));
    }
    return w[0] >= 0 && w[1] >= 0 && w[2] >= 0;
}

// perspective-correct depth (one rounding to fp32) and barycentrics b[k] (fp64)
__device__ __forceinline__ float tri_depth(const Tri& t, const long long (&w)[3], double (&b)[3]) {
    double r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = ((double)w[k] / t.area) / t.z[k];
    const double q = (r[0] + r[1]) + r[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = r[k] / q;
    return (float)(1.0 / q);
}

__device__ __forceinline__ void tri_sample(const Tri& t, long long f, long long i, long long j, int W, unsigned long long* __restrict__ zbuf) {
    long long w[3];
    if (!tri_weights(t, i, j, w)) return;
    double b[3];
    const float depth = tri_depth(t, w, b);
    atomicMin(&zbuf[j * W + i], ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)f);
}

// One lane per face: set it up, count it, walk a small box here or put the face on the wave list.
__global__ __launch_bounds__(256) void k_raster_setup(const int* __restrict__ faces, long long n_faces, long long n_verts,
                                                      const ProjVert* __restrict__ pv, int H, int W, int wave_min_pixels,
                                                      unsigned long long* __restrict__ zbuf, int* __restrict__ list, unsigned* __restrict__ list_count,
                                                      unsigned long long* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    Tri t;
    const int kind = f < n_faces ? tri_setup(faces, f, n_verts, pv, H, W, t) : -1;
    const bool to_wave = kind == kFaceDrawn && wave_min_pixels != INT32_MAX && t.npix >= (long long)wave_min_pixels;
    // the four counters: one atomic per wavefront and counter (sums: the same whatever the order)
    const unsigned long long votes[4] = {__ballot(kind == kFaceDrawn), __ballot(kind == kFaceCulled), __ballot(kind == kFaceDegenerate), __ballot(to_wave)};
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (votes[k]) atomicAdd(&counts[k], (unsigned long long)__popcll(votes[k]));
    }
    // the wave list: one atomicAdd per wavefront reserves its slots
    if (votes[3]) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(list_count, (unsigned)__popcll(votes[3]));
        base = __shfl(base, 0);
        if (to_wave) list[base + __popcll(votes[3] & ((1ull << lane) - 1ull))] = (int)f;
    }
    if (kind != kFaceDrawn || to_wave) return;
    for (long long j = t.j0; j <= t.j1; ++j)
        for (long long i = t.i0; i <= t.i1; ++i) tri_sample(t, f, i, j, W, zbuf);
}

// One wavefront per listed face, lanes striding over its box; the fixed grid strides over the list.
__global__ __launch_bounds__(256) void k_raster_wave(const int* __restrict__ faces, long long n_faces, long long n_verts, const ProjVert* __restrict__ pv,
                                                     int H, int W, unsigned long long* __restrict__ zbuf, const int* __restrict__ list,
                                                     const unsigned* __restrict__ list_count) {
    const long long n = min((long long)list_count[0], n_faces);
    const int lane = threadIdx.x & 63;
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += (long long)gridDim.x * 4) {
        const long long f = list[e];
        if (f < 0 || f >= n_faces) continue;
        Tri t;
        if (tri_setup(faces, f, n_verts, pv, H, W, t) != kFaceDrawn) continue;
        const unsigned bw = (unsigned)(t.i1 - t.i0 + 1), npix = (unsigned)t.npix;       // npix <= H W < 2^31 (an empty box: npix = 0, bw unused)
        for (unsigned p = lane; p < npix; p += 64) {
            const unsigned r = p / bw;
            tri_sample(t, f, t.i0 + (p - r * bw), t.j0 + r, W, zbuf);
        }
    }
}

// One lane per pixel: the winner's depth and face from the key, its weights recomputed from the same integers.
__global__ __launch_bounds__(256) void k_raster_resolve(const float* __restrict__ verts, const int* __restrict__ faces, long long n_faces,
                                                        long long n_verts, const float* __restrict__ attrs, int C, const ProjVert* __restrict__ pv,
                                                        const unsigned long long* __restrict__ zbuf, int H, int W, float fx, float fy, float cx,
                                                        float cy, const float* __restrict__ c2w, float* __restrict__ depth, int* __restrict__ face,
                                                        float* __restrict__ bary, float* __restrict__ attr_out, float* __restrict__ normal) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int j = (int)(p / W), i = (int)(p - (long long)j * W);
    const unsigned long long key = zbuf[p];
    const long long f = (long long)(key & 0xffffffffull);
    Tri t;
    long long w[3];
    // (a key this frame's mofa_raster_faces wrote names a face that covers the pixel; anything else is left empty, never followed)
    const bool hit = key != kEmpty && f < n_faces && tri_setup(faces, f, n_verts, pv, H, W, t) == kFaceDrawn && tri_weights(t, i, j, w);
    double b[3] = {0.0, 0.0, 0.0};
    if (hit) tri_depth(t, w, b);
    depth[p] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    face[p] = hit ? (int)f : -1;
    if (bary) {
#pragma unroll
        for (int k = 0; k < 3; ++k) bary[p * 3 + k] = (float)b[k];
    }
    const float* v[3] = {verts, verts, verts};
    long long vi[3] = {0, 0, 0};
    if (hit) {
#pragma unroll
        for (int k = 0; k < 3; ++k) vi[k] = faces[f * 3 + k], v[k] = verts + vi[k] * 3;
    }
    if (attr_out) {
        for (int c = 0; c < C; ++c) {
            float a = 0.0f;
            if (hit)
                a = (float)((b[0] * (double)attrs[vi[0] * C + c] + b[1] * (double)attrs[vi[1] * C + c]) + b[2] * (double)attrs[vi[2] * C + c]);
            attr_out[p * C + c] = a;
        }
    }
    if (normal) {
        float n[3] = {0.f, 0.f, 0.f};
        if (hit) {
            float du[3], dv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) du[k] = __fsub_rn(v[1][k], v[0][k]), dv[k] = __fsub_rn(v[2][k], v[0][k]);
            const float nx = __fsub_rn(__fmul_rn(du[1], dv[2]), __fmul_rn(du[2], dv[1]));
            const float ny = __fsub_rn(__fmul_rn(du[2], dv[0]), __fmul_rn(du[0], dv[2]));
            const float nz = __fsub_rn(__fmul_rn(du[0], dv[1]), __fmul_rn(du[1], dv[0]));
            // sqrtf: the correctly rounded square root (as in k_point_normals)
            const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
            if (len > 0.f) {
                n[0] = __fdiv_rn(nx, len), n[1] = __fdiv_rn(ny, len), n[2] = __fdiv_rn(nz, len);
                float ro[3], rd[3];
                pinhole_ray(i, j, fx, fy, cx, cy, c2w, ro, rd);
                const float s = __fadd_rn(__fadd_rn(__fmul_rn(n[0], rd[0]), __fmul_rn(n[1], rd[1])), __fmul_rn(n[2], rd[2]));
                if (s > 0.f) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) normal[p * 3 + k] = n[k];
    }
}

}  // namespace
}  // namespace mofa

using namespace mofa;

extern "C" {

size_t mofa_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t H, int32_t W) {
    if (!raster_sizes_ok(n_verts, n_faces, H, W)) return 0;
    return raster_ws(nullptr, n_verts, n_faces, H, W).bytes;
}

int mofa_raster_project(const float* verts, int64_t n_verts, int64_t n_faces, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                        const float* c2w, float znear, void* workspace, void* stream) {
    MOFA_REQUIRE(raster_sizes_ok(n_verts, n_faces, H, W), "raster_project: %lld vertices, %lld faces, H = %d, W = %d (want H, W >= 1, H W < 2^31, 0 <= counts < 2^31)",
                 (long long)n_verts, (long long)n_faces, H, W);
    MOFA_REQUIRE(isfinite(znear) && znear > 0.f, "raster_project: znear = %g (want finite and > 0)", (double)znear);
    MOFA_REQUIRE(c2w && workspace && (verts || n_verts == 0), "raster_project: null pointer");
    if (n_verts == 0) return MOFA_OK;
    const RasterWs w = raster_ws(workspace, n_verts, n_faces, H, W);
    hipLaunchKernelGGL(k_raster_project, dim3(blocks_of(n_verts)), dim3(256), 0, (hipStream_t)stream, verts, (long long)n_verts, c2w, fx, fy, cx, cy,
                       znear, w.pv);
    return check_launch("k_raster_project");
}

int mofa_raster_faces(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t H, int32_t W, int32_t wave_min_pixels, void* workspace,
                      int64_t* counts, void* stream) {
    MOFA_REQUIRE(raster_sizes_ok(n_verts, n_faces, H, W), "raster_faces: %lld vertices, %lld faces, H = %d, W = %d (want H, W >= 1, H W < 2^31, 0 <= counts < 2^31)",
                 (long long)n_verts, (long long)n_faces, H, W);
    MOFA_REQUIRE(wave_min_pixels >= 0, "raster_faces: wave_min_pixels = %d (want >= 0)", wave_min_pixels);
    MOFA_REQUIRE(workspace && counts && (faces || n_faces == 0), "raster_faces: null pointer");
    const RasterWs w = raster_ws(workspace, n_verts, n_faces, H, W);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_raster_clear, dim3(blocks_of((long long)H * W)), dim3(256), 0, st, w.zbuf, (long long)H * W, w.list_count,
                       (unsigned long long*)counts);
    int rc = check_launch("k_raster_clear");
    if (rc != MOFA_OK || n_faces == 0) return rc;
    hipLaunchKernelGGL(k_raster_setup, dim3(blocks_of(n_faces)), dim3(256), 0, st, faces, (long long)n_faces, (long long)n_verts, w.pv, (int)H, (int)W,
                       (int)wave_min_pixels, w.zbuf, w.list, w.list_count, (unsigned long long*)counts);
    if ((rc = check_launch("k_raster_setup")) != MOFA_OK) return rc;
    if (wave_min_pixels == INT32_MAX) return MOFA_OK;          // nothing can be on the list
    hipLaunchKernelGGL(k_raster_wave, dim3(kWaveBlocks), dim3(256), 0, st, faces, (long long)n_faces, (long long)n_verts, w.pv, (int)H, (int)W, w.zbuf,
                       w.list, w.list_count);
    return check_launch("k_raster_wave");
}

int mofa_raster_resolve(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* attrs, int32_t C, int32_t H,
                        int32_t W, float fx, float fy, float cx, float cy, const float* c2w, const void* workspace, float* depth, int32_t* face,
                        float* bary, float* attr_out, float* normal, void* stream) {
    MOFA_REQUIRE(raster_sizes_ok(n_verts, n_faces, H, W), "raster_resolve: %lld vertices, %lld faces, H = %d, W = %d (want H, W >= 1, H W < 2^31, 0 <= counts < 2^31)",
                 (long long)n_verts, (long long)n_faces, H, W);
    MOFA_REQUIRE(!attr_out || (C >= 1 && C <= 16), "raster_resolve: C = %d attributes per vertex (want 1 .. 16)", C);
    MOFA_REQUIRE(!attr_out || attrs || n_verts == 0, "raster_resolve: attr_out without attrs");
    MOFA_REQUIRE(c2w && workspace && depth && face && (verts || n_verts == 0) && (faces || n_faces == 0), "raster_resolve: null pointer");
    const RasterWs w = raster_ws(const_cast<void*>(workspace), n_verts, n_faces, H, W);
    hipLaunchKernelGGL(k_raster_resolve, dim3(blocks_of((long long)H * W)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)n_faces,
                       (long long)n_verts, attrs, (int)C, w.pv, w.zbuf, (int)H, (int)W, fx, fy, cx, cy, c2w, depth, face, bary, attr_out, normal);
    return check_launch("k_raster_resolve");
}

}  // extern "C"
