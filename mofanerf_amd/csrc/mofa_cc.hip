// Connected components of a triangle mesh for the geometry export (gfx950): labels by shared vertex index, per-component statistics
// and the face side of a compaction.  mesh.py drives the passes; nothing here waits on another thread.
//
//   validate    counts[0] += face indices outside [0, V): the caller reads it and launches nothing else when it is not zero.  Every
//               kernel below checks the indices it dereferences all the same (a bad face is skipped), so a bad index is never a fault.
//   labels      parent[v] = v; then passes of  hook: for the edges (a, b), (b, c) of every face, ra = root(a), rb = root(b);
//               ra != rb -> atomicMin(&parent[max(ra, rb)], min(ra, rb)), *changed = 1   and   compress: parent[v] = root(v)
//               until a pass changes nothing.  Every write to parent[] lowers it, so parent[x] <= x always holds and the root walk
//               x = parent[x] strictly decreases: it is the only loop here whose trip count depends on the data, and it ends by itself.
//               A racing atomicMin can cut a link another thread just made; that pass has then changed something, and the next one
//               hooks the edge again.  At the fixed point root(a) == root(b) for every edge and the root is the component's smallest
//               vertex index whatever the arrival order.  Integer atomicMin only: the labels are the same bits every time.
//   terms       per face, in fp64 from the fp32 coordinates, every operation rounded separately:
//               area 0.5 |(v1 - v0) x (v2 - v0)|, volume v0 . (v1 x v2) / 6 (signed: > 0 for a solid with normals toward lower density)
//   seg_sum     out[s] = the sum of rows [seg_start[s], seg_end[s]) of in[N,2] (through perm, if given): one workgroup per segment, thread t
//               adds rows t, t + 256, ... in that order, then a fixed tree over the 256 partial sums.  The caller sums each label's
//               run of label-sorted faces in chunks of 1024 (mesh.CC_CHUNK), then each label's chunks: a fixed order at both levels, the same bits.
//   seg_minmax  the same walk with min / max over points [N,3] or boxes [N,2,3], compared as the order-preserving integer key of a float:
//               the exact per-component box from the vertices sorted by label, two levels, no atomics
//   remap       out[i] = vmap[in[i]] for the face indices of a compaction (-1 for an index outside [0, V))
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kCcMaxIndex = (1ll << 31) - 1;     // V, F and every element count of a launch: int32 indices, one thread per element

__device__ __forceinline__ bool cc_in_range(int v, int V) { return (unsigned)v < (unsigned)V; }

// the root of x: follow parent[] while it decreases.  x is in [0, V); a value that does not decrease (a root, or garbage) ends the walk,
// so every index read is one already checked and the walk takes at most x steps.
__device__ __forceinline__ int cc_root(const int* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

__global__ __launch_bounds__(256) void k_cc_validate(const int* __restrict__ faces, long long F, int V, int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int bad = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) bad += !cc_in_range(faces[f * 3 + c], V);
    if (bad) atomicAdd((unsigned long long*)counts, (unsigned long long)bad);
}

__global__ __launch_bounds__(256) void k_cc_init(int* __restrict__ parent, int V) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V) parent[v] = (int)v;
}

// one edge: true when the roots differed (and the larger was hooked under the smaller)
__device__ __forceinline__ bool cc_hook_edge(int* parent, int a, int b) {
    const int ra = cc_root(parent, a), rb = cc_root(parent, b);
    if (ra == rb) return false;
    atomicMin(parent + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    return true;
}

__global__ __launch_bounds__(256) void k_cc_hook(const int* __restrict__ faces, long long F, int V, int* parent, int64_t* changed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (!cc_in_range(a, V) || !cc_in_range(b, V) || !cc_in_range(c, V)) return;
    const bool ab = cc_hook_edge(parent, a, b);
    const bool bc = cc_hook_edge(parent, b, c);
    if (ab || bc) __hip_atomic_store(changed, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_cc_compress(int* parent, int V) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int r = cc_root(parent, (int)v);
    if (r != (int)v) atomicMin(parent + v, r);       // (an atomic like every other write to parent[]: it can only lower the entry)
}

// float bits -> unsigned key with the order of the floats (-0 below +0)
__device__ __forceinline__ unsigned cc_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cc_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void k_cc_face_terms(const float* __restrict__ verts, const int* __restrict__ faces, long long F, int V,
                                                       double* __restrict__ terms) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (!cc_in_range(i0, V) || !cc_in_range(i1, V) || !cc_in_range(i2, V)) {
        terms[f * 2 + 0] = 0.0, terms[f * 2 + 1] = 0.0;
        return;
    }
    double p[3], q[3], r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (double)verts[(long long)i0 * 3 + c], q[c] = (double)verts[(long long)i1 * 3 + c], r[c] = (double)verts[(long long)i2 * 3 + c];
    const double ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
    const double wx = r[0] - p[0], wy = r[1] - p[1], wz = r[2] - p[2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    terms[f * 2 + 0] = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
    const double cx = q[1] * r[2] - q[2] * r[1], cy = q[2] * r[0] - q[0] * r[2], cz = q[0] * r[1] - q[1] * r[0];
    terms[f * 2 + 1] = ((p[0] * cx + p[1] * cy) + p[2] * cz) / 6.0;
}

// `iters` (from the host: ceil(longest segment / 256)) fixes the trip count; the segment's own ends only mask rows out
__global__ __launch_bounds__(256) void k_cc_seg_sum(const double* __restrict__ in, const int64_t* __restrict__ perm, long long N,
                                                    const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end, int iters,
                                                    double* __restrict__ out) {
    __shared__ double sm[2][256];
    const long long s = blockIdx.x;
    long long s0 = seg_start[s], s1 = seg_end[s];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > N ? N : s1;
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < iters; ++k) {
        const long long i = s0 + t + (long long)k * 256;
        if (i < s1) {
            long long row = perm ? perm[i] : i;
            if (row >= 0 && row < N) a += in[row * 2 + 0], b += in[row * 2 + 1];
        }
    }
    sm[0][t] = a, sm[1][t] = b;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) sm[0][t] += sm[0][t + w], sm[1][t] += sm[1][t + w];
        __syncthreads();
    }
    if (t == 0) out[s * 2 + 0] = sm[0][0], out[s * 2 + 1] = sm[1][0];
}

// the same walk for boxes: out[s] = [min xyz, max xyz] over the segment's rows of in — points [N,3] (BOXES = false) or boxes [N,2,3] —
// compared as the floats' order-preserving keys, so -0 < +0 and the result does not depend on who compares first
template <bool BOXES>
__global__ __launch_bounds__(256) void k_cc_seg_minmax(const float* __restrict__ in, const int64_t* __restrict__ perm, long long N,
                                                       const int64_t* __restrict__ seg_start, const int64_t* __restrict__ seg_end, int iters,
                                                       float* __restrict__ out) {
    __shared__ unsigned sm[6][256];
    const long long s = blockIdx.x;
    long long s0 = seg_start[s], s1 = seg_end[s];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > N ? N : s1;
    const int t = threadIdx.x;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (int k = 0; k < iters; ++k) {
        const long long i = s0 + t + (long long)k * 256;
        if (i < s1) {
            const long long row = perm ? perm[i] : i;
            if (row >= 0 && row < N) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned l = cc_key(in[row * (BOXES ? 6 : 3) + c]), h = BOXES ? cc_key(in[row * 6 + 3 + c]) : l;
                    lo[c] = l < lo[c] ? l : lo[c];
                    hi[c] = h > hi[c] ? h : hi[c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) sm[c][t] = lo[c], sm[3 + c][t] = hi[c];
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sm[c][t] = sm[c][t + w] < sm[c][t] ? sm[c][t + w] : sm[c][t];
                sm[3 + c][t] = sm[3 + c][t + w] > sm[3 + c][t] ? sm[3 + c][t + w] : sm[3 + c][t];
            }
        }
        __syncthreads();
    }
    if (t < 6) out[s * 6 + t] = cc_unkey(sm[t][0]);
}

__global__ __launch_bounds__(256) void k_cc_remap(const int* __restrict__ in, long long n, const int* __restrict__ vmap, int V,
                                                  int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = in[i];
    out[i] = cc_in_range(v, V) ? vmap[v] : -1;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_CC_COUNT(what, name, n) \
    MOFA_REQUIRE((n) >= 1 && (n) <= kCcMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

extern "C" {

int mofa_cc_validate(const int32_t* faces, int64_t F, int64_t V, int64_t* counts, void* stream) {
    MOFA_REQUIRE(faces && counts, "cc_validate: null pointer");
    MOFA_CC_COUNT("cc_validate", "F", F);
    MOFA_CC_COUNT("cc_validate", "V", V);
    hipLaunchKernelGGL(k_cc_validate, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, faces, (long long)F, (int)V, counts);
    return check_launch("k_cc_validate");
}

int mofa_cc_init(int32_t* parent, int64_t V, void* stream) {
    MOFA_REQUIRE(parent, "cc_init: null pointer");
    MOFA_CC_COUNT("cc_init", "V", V);
    hipLaunchKernelGGL(k_cc_init, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, parent, (int)V);
    return check_launch("k_cc_init");
}

int mofa_cc_hook(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int64_t* changed, void* stream) {
    MOFA_REQUIRE(faces && parent && changed, "cc_hook: null pointer");
    MOFA_CC_COUNT("cc_hook", "F", F);
    MOFA_CC_COUNT("cc_hook", "V", V);
    hipLaunchKernelGGL(k_cc_hook, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, faces, (long long)F, (int)V, parent, changed);
    return check_launch("k_cc_hook");
}

int mofa_cc_compress(int32_t* parent, int64_t V, void* stream) {
    MOFA_REQUIRE(parent, "cc_compress: null pointer");
    MOFA_CC_COUNT("cc_compress", "V", V);
    hipLaunchKernelGGL(k_cc_compress, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, parent, (int)V);
    return check_launch("k_cc_compress");
}

int mofa_cc_face_terms(const float* verts, const int32_t* faces, int64_t F, int64_t V, double* terms, void* stream) {
    MOFA_REQUIRE(verts && faces && terms, "cc_face_terms: null pointer");
    MOFA_CC_COUNT("cc_face_terms", "F", F);
    MOFA_CC_COUNT("cc_face_terms", "V", V);
    hipLaunchKernelGGL(k_cc_face_terms, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, verts, faces, (long long)F, (int)V, terms);
    return check_launch("k_cc_face_terms");
}

int mofa_cc_seg_sum(const double* in, const int64_t* perm, int64_t N, const int64_t* seg_start, const int64_t* seg_end, int64_t n_segments,
                    int64_t longest, double* out, void* stream) {
    MOFA_REQUIRE(in && seg_start && seg_end && out, "cc_seg_sum: null pointer");
    MOFA_CC_COUNT("cc_seg_sum", "N", N);
    MOFA_CC_COUNT("cc_seg_sum", "n_segments", n_segments);
    MOFA_REQUIRE(longest >= 0 && longest <= kCcMaxIndex, "cc_seg_sum: longest = %lld (want 0 .. 2^31 - 1)", (long long)longest);
    const int iters = (int)((longest + 255) / 256);
    hipLaunchKernelGGL(k_cc_seg_sum, dim3((unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, in, perm, (long long)N, seg_start, seg_end,
                       iters, out);
    return check_launch("k_cc_seg_sum");
}

int mofa_cc_seg_minmax(const float* in, int32_t boxes, const int64_t* perm, int64_t N, const int64_t* seg_start, const int64_t* seg_end,
                       int64_t n_segments, int64_t longest, float* out, void* stream) {
    MOFA_REQUIRE(in && seg_start && seg_end && out, "cc_seg_minmax: null pointer");
    MOFA_CC_COUNT("cc_seg_minmax", "N", N);
    MOFA_CC_COUNT("cc_seg_minmax", "n_segments", n_segments);
    MOFA_REQUIRE(longest >= 0 && longest <= kCcMaxIndex, "cc_seg_minmax: longest = %lld (want 0 .. 2^31 - 1)", (long long)longest);
    const int iters = (int)((longest + 255) / 256);
    if (boxes)
        hipLaunchKernelGGL(k_cc_seg_minmax<true>, dim3((unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, in, perm, (long long)N, seg_start,
                           seg_end, iters, out);
    else
        hipLaunchKernelGGL(k_cc_seg_minmax<false>, dim3((unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, in, perm, (long long)N, seg_start,
                           seg_end, iters, out);
    return check_launch("k_cc_seg_minmax");
}

int mofa_cc_remap(const int32_t* in, int64_t n, const int32_t* vmap, int64_t V, int32_t* out, void* stream) {
    MOFA_REQUIRE(in && vmap && out, "cc_remap: null pointer");
    MOFA_REQUIRE(n >= 1 && n <= 3 * kCcMaxIndex, "cc_remap: n = %lld (want 1 .. 3 (2^31 - 1))", (long long)n);
    MOFA_CC_COUNT("cc_remap", "V", V);
    hipLaunchKernelGGL(k_cc_remap, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, in, (long long)n, vmap, (int)V, out);
    return check_launch("k_cc_remap");
}

}  // extern "C"
