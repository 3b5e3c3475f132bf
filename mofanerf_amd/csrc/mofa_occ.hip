// Occupancy-culled rendering (gfx950): an occupancy grid over the lattice of mofa_grid_points, the classification of a pass's samples
// against it, their compaction into the explicit points the network is given, and the scatter of the network's values back into raw.
// Deterministic with no atomics: a kept sample's slot is the 64-bit exclusive scan of the flags (mofa_mesh.hip's scan), so the kept
// list is in ascending (ray, sample) order and the same input gives the same bytes.
//
//   cells      lattice nx x ny x nz -> (nx-1)(ny-1)(nz-1) cells, cell c = (i * (ny-1) + j) * (nz-1) + k, one byte each;
//              occupied iff one of the 8 corner samples is > threshold (false for NaN); dilation = separable maximum over [-d, d]
//   point      p = o + d * z, multiply and add rounded separately (the bits the network's own prologue forms)
//   per axis   t = (p - lo) / step (correctly rounded);  inside = t >= 0 && t <= (float)(n - 1) (false for NaN);  c = min((int)t, n - 2)
//   kept       inside on all three axes and the cell occupied
//
// Kernels: k_occ_cells, k_occ_dilate_axis, k_occ_classify, k_occ_total, k_occ_gather, k_occ_scatter, k_occ_scatter_sigma.  One lane per cell / sample.
#include <math.h>

#include "mofa_common.h"

extern "C" {
// mofa_mesh.hip: the 64-bit exclusive scan of byte counts and the elements of scratch it needs
long long mofa_internal_scan_aux(long long n);
int mofa_internal_scan_bytes(const unsigned char* in, long long n, long long* out, long long* aux, void* stream);
}

namespace mofa {
namespace {

constexpr long long kOccMaxSamples = 1ll << 31;      // samples of one pass: the kept list holds int32 sample indices
constexpr long long kOccMaxCells = 1ll << 31;
constexpr int kOccMaxDilate = 8;

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }
inline size_t align_up(size_t v) { return (v + 255) / 256 * 256; }

bool occ_grid_ok(long long nx, long long ny, long long nz) {
    if (nx < 2 || ny < 2 || nz < 2 || nx >= (1ll << 24) || ny >= (1ll << 24) || nz >= (1ll << 24)) return false;
    if ((nx - 1) * (ny - 1) >= kOccMaxCells) return false;
    return (nx - 1) * (ny - 1) * (nz - 1) < kOccMaxCells;
}

struct OccGrid {
    int nx, ny, nz;          // lattice samples per axis
    float lox, loy, loz, sx, sy, sz;
};

__global__ __launch_bounds__(256) void k_occ_cells(const float* __restrict__ grid, long long ny, long long nz, long long n_cells,
                                                   float threshold, int merge, unsigned char* __restrict__ cells) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const long long cy = ny - 1, cz = nz - 1;
    const long long i = c / (cy * cz), r = c - i * (cy * cz), j = r / cz, k = r - j * cz;
    bool occ = false;
#pragma unroll
    for (int b = 0; b < 8; ++b) occ |= grid[((i + (b & 1)) * ny + j + ((b >> 1) & 1)) * nz + k + (b >> 2)] > threshold;
    if (merge) occ |= cells[c] != 0;
    cells[c] = occ ? 1 : 0;
}

// out[c] = maximum of in over the cells within `d` of c along `axis` (0: x, 1: y, 2: z), clipped at the borders
__global__ __launch_bounds__(256) void k_occ_dilate_axis(const unsigned char* __restrict__ in, long long cx, long long cy, long long cz, int axis,
                                                         int d, unsigned char* __restrict__ out) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cx * cy * cz) return;
    const long long i = c / (cy * cz), r = c - i * (cy * cz), j = r / cz, k = r - j * cz;
    const long long pos = axis == 0 ? i : (axis == 1 ? j : k), len = axis == 0 ? cx : (axis == 1 ? cy : cz);
    const long long stride = axis == 0 ? cy * cz : (axis == 1 ? cz : 1);
    const long long a = pos - d < 0 ? 0 : pos - d, b = pos + d > len - 1 ? len - 1 : pos + d;
    unsigned char occ = 0;
    for (long long q = a; q <= b; ++q) occ |= in[c + (q - pos) * stride];
    out[c] = occ ? 1 : 0;
}

// one axis of the classification: inside the lattice's span, and the cell coordinate
__device__ __forceinline__ bool occ_axis(float p, float lo, float step, int n, int& c) {
    const float t = __fdiv_rn(__fsub_rn(p, lo), step);
    if (!(t >= 0.0f && t <= (float)(n - 1))) return false;          // (NaN: outside)
    const int ci = (int)t;
    c = ci < n - 2 ? ci : n - 2;
    return true;
}

__device__ __forceinline__ float occ_point(float o, float d, float z) { return __fadd_rn(o, __fmul_rn(d, z)); }

__global__ __launch_bounds__(256) void k_occ_classify(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                      const float* __restrict__ z, long long z_row_stride, long long n_samples, int S,
                                                      const unsigned char* __restrict__ cells, OccGrid g, unsigned char* __restrict__ flags) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples) return;
    const long long r = e / S;
    const int s = (int)(e - r * S);
    const float zv = z[r * z_row_stride + s];
    int ci, cj, ck;
    bool keep = occ_axis(occ_point(rays_o[r * 3 + 0], rays_d[r * 3 + 0], zv), g.lox, g.sx, g.nx, ci);
    keep = occ_axis(occ_point(rays_o[r * 3 + 1], rays_d[r * 3 + 1], zv), g.loy, g.sy, g.ny, cj) && keep;
    keep = occ_axis(occ_point(rays_o[r * 3 + 2], rays_d[r * 3 + 2], zv), g.loz, g.sz, g.nz, ck) && keep;
    if (keep) keep = cells[((long long)ci * (g.ny - 1) + cj) * (g.nz - 1) + ck] != 0;
    flags[e] = keep ? 1 : 0;
}

__global__ void k_occ_total(const long long* __restrict__ scan, const unsigned char* __restrict__ flags, long long n, long long* __restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counts[0] = scan[n - 1] + flags[n - 1];
}

__global__ __launch_bounds__(256) void k_occ_gather(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                    const float* __restrict__ viewdirs, const float* __restrict__ z, long long z_row_stride,
                                                    long long n_samples, int S, const unsigned char* __restrict__ flags,
                                                    const long long* __restrict__ scan, long long n_kept, float* __restrict__ pts,
                                                    float* __restrict__ dirs, int* __restrict__ index) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples || !flags[e]) return;
    const long long k = scan[e];
    if (k >= n_kept) return;                            // (the caller's count does not belong to these flags: write nothing)
    const long long r = e / S;
    const int s = (int)(e - r * S);
    const float zv = z[r * z_row_stride + s];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pts[k * 3 + a] = occ_point(rays_o[r * 3 + a], rays_d[r * 3 + a], zv);
        dirs[k * 3 + a] = viewdirs[r * 3 + a];
    }
    index[k] = (int)e;
}

// every element of raw: the network's four values for a kept sample, zeros for a skipped one
__global__ __launch_bounds__(256) void k_occ_scatter(const f32x4* __restrict__ raw_kept, const unsigned char* __restrict__ flags,
                                                     const long long* __restrict__ scan, long long n_samples, long long n_kept,
                                                     f32x4* __restrict__ raw) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples) return;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (flags[e]) {
        const long long k = scan[e];
        const float bad = __builtin_nanf("");
        v = k < n_kept ? raw_kept[k] : f32x4{bad, bad, bad, bad};
    }
    raw[e] = v;
}

// the one-float twin (the geometry-only render): every element of sigma, the network's density for a kept sample, zero for a skipped one
__global__ __launch_bounds__(256) void k_occ_scatter_sigma(const float* __restrict__ sigma_kept, const unsigned char* __restrict__ flags,
                                                           const long long* __restrict__ scan, long long n_samples, long long n_kept,
                                                           float* __restrict__ sigma) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples) return;
    float v = 0.0f;
    if (flags[e]) {
        const long long k = scan[e];
        v = k < n_kept ? sigma_kept[k] : __builtin_nanf("");
    }
    sigma[e] = v;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_OCC_GRID(what)                                                                                                                    \
    MOFA_REQUIRE(occ_grid_ok(nx, ny, nz), what ": lattice %lld x %lld x %lld is refused (2 <= n < 2^24 per axis, fewer than 2^31 cells)",        \
                 (long long)nx, (long long)ny, (long long)nz)
#define MOFA_OCC_PASS(what)                                                                                                                    \
    MOFA_REQUIRE(n_rays >= 1 && S >= 1 && n_rays < kOccMaxSamples && n_rays * (int64_t)S < kOccMaxSamples,                                      \
                 what ": %lld rays x %d samples (want at least one and fewer than 2^31 samples)", (long long)n_rays, (int)S);                   \
    MOFA_REQUIRE(z_row_stride == 0 || z_row_stride >= S, what ": z_row_stride = %lld with S = %d", (long long)z_row_stride, (int)S)

extern "C" {

size_t mofa_occ_workspace_bytes(int64_t n_samples) {
    if (n_samples < 1 || n_samples >= kOccMaxSamples) return 0;
    return align_up((size_t)n_samples * 8) + align_up((size_t)mofa_internal_scan_aux(n_samples) * 8);
}

int mofa_occ_cells(const float* grid, int64_t nx, int64_t ny, int64_t nz, float threshold, int32_t merge, uint8_t* cells, void* stream) {
    MOFA_REQUIRE(grid && cells, "occ_cells: null pointer");
    MOFA_OCC_GRID("occ_cells");
    MOFA_REQUIRE(isfinite(threshold), "occ_cells: the threshold must be finite (got %g)", (double)threshold);
    const long long n_cells = (nx - 1) * (ny - 1) * (nz - 1);
    hipLaunchKernelGGL(k_occ_cells, dim3(blocks_of(n_cells)), dim3(256), 0, (hipStream_t)stream, grid, (long long)ny, (long long)nz, n_cells,
                       threshold, (int)merge, cells);
    return check_launch("k_occ_cells");
}

int mofa_occ_dilate(const uint8_t* cells, int64_t nx, int64_t ny, int64_t nz, int32_t dilate, uint8_t* scratch, uint8_t* out, void* stream) {
    MOFA_REQUIRE(cells && scratch && out && cells != out && cells != scratch && scratch != out, "occ_dilate: null or aliased pointer");
    MOFA_OCC_GRID("occ_dilate");
    MOFA_REQUIRE(dilate >= 0 && dilate <= kOccMaxDilate, "occ_dilate: dilate = %d (want 0 .. %d cells)", (int)dilate, kOccMaxDilate);
    const long long cx = nx - 1, cy = ny - 1, cz = nz - 1;
    const dim3 grid(blocks_of(cx * cy * cz));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_occ_dilate_axis, grid, dim3(256), 0, st, (const unsigned char*)cells, cx, cy, cz, 0, (int)dilate, out);
    hipLaunchKernelGGL(k_occ_dilate_axis, grid, dim3(256), 0, st, (const unsigned char*)out, cx, cy, cz, 1, (int)dilate, scratch);
    hipLaunchKernelGGL(k_occ_dilate_axis, grid, dim3(256), 0, st, (const unsigned char*)scratch, cx, cy, cz, 2, (int)dilate, out);
    return check_launch("k_occ_dilate_axis");
}

int mofa_occ_classify(const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride, int64_t n_rays, int32_t S,
                      const uint8_t* cells, int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], uint8_t* flags,
                      void* workspace, int64_t* counts, void* stream) {
    MOFA_REQUIRE(rays_o && rays_d && z && cells && lo && step && flags && workspace && counts, "occ_classify: null pointer");
    MOFA_OCC_GRID("occ_classify");
    MOFA_OCC_PASS("occ_classify");
    for (int a = 0; a < 3; ++a)
        MOFA_REQUIRE(isfinite(lo[a]) && isfinite(step[a]) && step[a] > 0, "occ_classify: lo[%d] = %g, step[%d] = %g (want finite, step > 0)", a,
                     (double)lo[a], a, (double)step[a]);
    const long long n = (long long)n_rays * S;
    const OccGrid g{(int)nx, (int)ny, (int)nz, lo[0], lo[1], lo[2], step[0], step[1], step[2]};
    long long* scan = (long long*)workspace;
    long long* aux = (long long*)((char*)workspace + align_up((size_t)n * 8));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_occ_classify, dim3(blocks_of(n)), dim3(256), 0, st, rays_o, rays_d, z, (long long)z_row_stride, n, (int)S,
                       (const unsigned char*)cells, g, (unsigned char*)flags);
    int rc = check_launch("k_occ_classify");
    if (rc != MOFA_OK) return rc;
    if ((rc = mofa_internal_scan_bytes((const unsigned char*)flags, n, scan, aux, stream)) != MOFA_OK) return rc;
    hipLaunchKernelGGL(k_occ_total, dim3(1), dim3(64), 0, st, (const long long*)scan, (const unsigned char*)flags, n, (long long*)counts);
    return check_launch("k_occ_total");
}

int mofa_occ_gather(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z, int64_t z_row_stride, int64_t n_rays,
                    int32_t S, const uint8_t* flags, const void* workspace, int64_t n_kept, float* pts, float* dirs, int32_t* index,
                    void* stream) {
    MOFA_REQUIRE(rays_o && rays_d && viewdirs && z && flags && workspace && pts && dirs && index, "occ_gather: null pointer");
    MOFA_OCC_PASS("occ_gather");
    const long long n = (long long)n_rays * S;
    MOFA_REQUIRE(n_kept >= 1 && n_kept <= n, "occ_gather: n_kept = %lld of %lld samples", (long long)n_kept, n);
    hipLaunchKernelGGL(k_occ_gather, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, viewdirs, z, (long long)z_row_stride,
                       n, (int)S, (const unsigned char*)flags, (const long long*)workspace, (long long)n_kept, pts, dirs, (int*)index);
    return check_launch("k_occ_gather");
}

int mofa_occ_scatter(const float* raw_kept, const uint8_t* flags, const void* workspace, int64_t n_samples, int64_t n_kept, float* raw,
                     void* stream) {
    MOFA_REQUIRE(flags && workspace && raw, "occ_scatter: null pointer");
    MOFA_REQUIRE(n_samples >= 1 && n_samples < kOccMaxSamples, "occ_scatter: %lld samples", (long long)n_samples);
    MOFA_REQUIRE(n_kept >= 0 && n_kept <= n_samples && (n_kept == 0 || raw_kept), "occ_scatter: n_kept = %lld of %lld samples (raw_kept %s)",
                 (long long)n_kept, (long long)n_samples, raw_kept ? "given" : "NULL");
    MOFA_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)raw_kept & 15) == 0, "occ_scatter: raw and raw_kept must be 16-byte aligned");
    hipLaunchKernelGGL(k_occ_scatter, dim3(blocks_of(n_samples)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)raw_kept,
                       (const unsigned char*)flags, (const long long*)workspace, (long long)n_samples, (long long)n_kept, (f32x4*)raw);
    return check_launch("k_occ_scatter");
}

int mofa_occ_scatter_sigma(const float* sigma_kept, const uint8_t* flags, const void* workspace, int64_t n_samples, int64_t n_kept,
                           float* sigma, void* stream) {
    MOFA_REQUIRE(flags && workspace && sigma, "occ_scatter_sigma: null pointer");
    MOFA_REQUIRE(n_samples >= 1 && n_samples < kOccMaxSamples, "occ_scatter_sigma: %lld samples", (long long)n_samples);
    MOFA_REQUIRE(n_kept >= 0 && n_kept <= n_samples && (n_kept == 0 || sigma_kept),
                 "occ_scatter_sigma: n_kept = %lld of %lld samples (sigma_kept %s)", (long long)n_kept, (long long)n_samples,
                 sigma_kept ? "given" : "NULL");
    hipLaunchKernelGGL(k_occ_scatter_sigma, dim3(blocks_of(n_samples)), dim3(256), 0, (hipStream_t)stream, sigma_kept,
                       (const unsigned char*)flags, (const long long*)workspace, (long long)n_samples, (long long)n_kept, sigma);
    return check_launch("k_occ_scatter_sigma");
}

}  // extern "C"
