// Mesh registration for the geometry export (gfx950): the estimation step of rigid / similarity ICP.  mesh.py drives the loop
// (mesh.register, mesh.fit_transform): it moves the points (apply), asks closest_points for the correspondences, decides the border rule
// (reject), and sums the normal equations of the linearised step (terms + reduce, or the two fused: terms_reduce); the 7 x 7 solve and the
// composition of the transform run on the host.  Nothing here waits on another thread and there is no atomic of any kind: every sum has
// a fixed order that does not depend on the launch geometry, so the same input gives the same bytes.  Every kernel checks the indices it
// dereferences; a correspondence with a bad one counts as rejected.  All arithmetic is fp64 on the fp32 inputs widened, every operation
// rounded separately (the build pins -ffp-contract=off).  The order of operations is the header's (include/mofanerf_hip.h); in short:
//
//   apply    out[i][r] = (float)(s * ((R[r][0] x0 + R[r][1] x1) + R[r][2] x2) + t[r])
//   terms    yh = y - mu;  d = y - c.
//              point:  J0 = [0, yh_z, -yh_y, 1, 0, 0, yh_x], J1 = [-yh_z, 0, yh_x, 0, 1, 0, yh_y], J2 = [yh_y, -yh_x, 0, 0, 0, 1, yh_z], r = d
//                      A_ab = w ((J0a J0b + J1a J1b) + J2a J2b),  g_a = w ((J0a r0 + J1a r1) + J2a r2),  e = w ((r0 r0 + r1 r1) + r2 r2)
//              plane:  J = [yh_y n_z - yh_z n_y, yh_z n_x - yh_x n_z, yh_x n_y - yh_y n_x, n_x, n_y, n_z, (n_x yh_x + n_y yh_y) + n_z yh_z],
//                      r = (n_x d_x + n_y d_y) + n_z d_z;  A_ab = w (Ja Jb),  g_a = w (Ja r),  e = w (r r)
//            36 numbers per correspondence: A's upper triangle row by row (28), g (7), e.  w > 0 is false: 36 exact zeros.
//   reduce   chunk k = rows [1024 k, 1024 (k + 1)): thread t of 256 starts from 0.0 and adds rows t, t + 256, t + 512, t + 768 of the chunk in
//            that order, then the tree `for w = 128, 64, .. 1: p[t] += p[t + w] (t < w)` runs over the 256 partial sums.  One row per chunk
//            comes out; the caller reduces those the same way until one row is left.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kIcpMaxIndex = (1ll << 31) - 1;     // N, V, F: int32 indices
constexpr int kIcpCols = MOFA_ICP_TERMS;                // 36
constexpr int kIcpChunk = MOFA_ICP_CHUNK;               // 1024 rows per workgroup: 4 per thread, a fixed trip count
constexpr int kIcpPass = 12;                            // columns per pass of the tree: 12 x 256 doubles of LDS

struct IcpTransform {
    double s, R[9], t[3];
};

__device__ __forceinline__ bool icp_in_range(int v, long long n) { return v >= 0 && (long long)v < n; }

__global__ __launch_bounds__(256) void k_icp_apply(const float* __restrict__ x, long long N, IcpTransform T, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double x0 = (double)x[i * 3 + 0], x1 = (double)x[i * 3 + 1], x2 = (double)x[i * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[i * 3 + r] = (float)(T.s * ((T.R[r * 3 + 0] * x0 + T.R[r * 3 + 1] * x1) + T.R[r * 3 + 2] * x2) + T.t[r]);
}

struct IcpInputs {
    const float* moved;       // y [N,3]
    const float* target;      // c [N,3]
    const float* normals;     // [N,3], or NULL: the normal of face[i]
    const int* face;          // [N], or NULL with `normals`
    const float* verts;       // [V,3]
    const int* faces;         // [F,3]
    const double* weight;     // [N]
    long long N, V, F;
    double mu[3];
};

// the 36 numbers of correspondence i; false (and zeros) when it is rejected
template <int PLANE>
__device__ __forceinline__ bool icp_row(const IcpInputs& in, long long i, double (&o)[kIcpCols]) {
#pragma unroll
    for (int j = 0; j < kIcpCols; ++j) o[j] = 0.0;
    const double w = in.weight[i];
    if (!(w > 0.0)) return false;
    double n[3] = {0.0, 0.0, 0.0};
    if (PLANE) {
        if (in.face) {
            const int f = in.face[i];
            if (!icp_in_range(f, in.F)) return false;
            const int ia = in.faces[(long long)f * 3 + 0], ib = in.faces[(long long)f * 3 + 1], ic = in.faces[(long long)f * 3 + 2];
            if (!icp_in_range(ia, in.V) || !icp_in_range(ib, in.V) || !icp_in_range(ic, in.V)) return false;
            double a[3], ab[3], ac[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a[k] = (double)in.verts[(long long)ia * 3 + k];
                ab[k] = (double)in.verts[(long long)ib * 3 + k] - a[k];
                ac[k] = (double)in.verts[(long long)ic * 3 + k] - a[k];
            }
            const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
            const double len = sqrt((cx * cx + cy * cy) + cz * cz);
            n[0] = cx / len, n[1] = cy / len, n[2] = cz / len;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = (double)in.normals[i * 3 + k];
        }
    }
    double yh[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double y = (double)in.moved[i * 3 + k];
        yh[k] = y - in.mu[k];
        d[k] = y - (double)in.target[i * 3 + k];
    }
    if (PLANE) {
        const double J[7] = {yh[1] * n[2] - yh[2] * n[1], yh[2] * n[0] - yh[0] * n[2], yh[0] * n[1] - yh[1] * n[0], n[0], n[1], n[2],
                             (n[0] * yh[0] + n[1] * yh[1]) + n[2] * yh[2]};
        const double r = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
        int j = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b) o[j++] = w * (J[a] * J[b]);
#pragma unroll
        for (int a = 0; a < 7; ++a) o[28 + a] = w * (J[a] * r);
        o[35] = w * (r * r);
    } else {
        const double J[3][7] = {{0.0, yh[2], -yh[1], 1.0, 0.0, 0.0, yh[0]}, {-yh[2], 0.0, yh[0], 0.0, 1.0, 0.0, yh[1]},
                                {yh[1], -yh[0], 0.0, 0.0, 0.0, 1.0, yh[2]}};
        int j = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b) o[j++] = w * ((J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b]);
#pragma unroll
        for (int a = 0; a < 7; ++a) o[28 + a] = w * ((J[0][a] * d[0] + J[1][a] * d[1]) + J[2][a] * d[2]);
        o[35] = w * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }
    return true;
}

template <int PLANE>
__global__ __launch_bounds__(256) void k_icp_terms(IcpInputs in, double* __restrict__ terms) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= in.N) return;
    double o[kIcpCols];
    icp_row<PLANE>(in, i, o);
#pragma unroll
    for (int j = 0; j < kIcpCols; ++j) terms[i * kIcpCols + j] = o[j];
}

// the tree over the workgroup's 256 partial sums of every column, kIcpPass columns at a time; thread 0 writes the chunk's row
__device__ __forceinline__ void icp_tree(double (&acc)[kIcpCols], int ncols, double* __restrict__ out_row) {
    __shared__ double sm[kIcpPass][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < kIcpCols / kIcpPass; ++p) {
#pragma unroll
        for (int j = 0; j < kIcpPass; ++j) sm[j][t] = acc[p * kIcpPass + j];
        __syncthreads();
#pragma unroll
        for (int w = 128; w >= 1; w >>= 1) {
            if (t < w) {
#pragma unroll
                for (int j = 0; j < kIcpPass; ++j) sm[j][t] += sm[j][t + w];
            }
            __syncthreads();
        }
        if (t < kIcpPass && p * kIcpPass + t < ncols) out_row[p * kIcpPass + t] = sm[t][0];
        __syncthreads();
    }
}

template <int PLANE>
__global__ __launch_bounds__(256) void k_icp_terms_reduce(IcpInputs in, double* __restrict__ partial) {
    const long long c0 = (long long)blockIdx.x * kIcpChunk;
    double acc[kIcpCols];
#pragma unroll
    for (int j = 0; j < kIcpCols; ++j) acc[j] = 0.0;
#pragma unroll 1
    for (int k = 0; k < kIcpChunk / 256; ++k) {
        const long long i = c0 + threadIdx.x + (long long)k * 256;
        if (i < in.N) {
            double o[kIcpCols];
            icp_row<PLANE>(in, i, o);
#pragma unroll
            for (int j = 0; j < kIcpCols; ++j) acc[j] += o[j];
        }
    }
    icp_tree(acc, kIcpCols, partial + (long long)blockIdx.x * kIcpCols);
}

__global__ __launch_bounds__(256) void k_icp_reduce(const double* __restrict__ in, long long M, int ncols, double* __restrict__ out) {
    const long long c0 = (long long)blockIdx.x * kIcpChunk;
    double acc[kIcpCols];
#pragma unroll
    for (int j = 0; j < kIcpCols; ++j) acc[j] = 0.0;
#pragma unroll 1
    for (int k = 0; k < kIcpChunk / 256; ++k) {
        const long long i = c0 + threadIdx.x + (long long)k * 256;
        if (i < M) {
#pragma unroll
            for (int j = 0; j < kIcpCols; ++j)
                if (j < ncols) acc[j] += in[i * ncols + j];
        }
    }
    icp_tree(acc, ncols, out + (long long)blockIdx.x * ncols);
}

__global__ __launch_bounds__(256) void k_icp_reject(const int* __restrict__ face, const float* __restrict__ bary, long long N,
                                                    const int* __restrict__ faces, long long F, long long V,
                                                    const uint8_t* __restrict__ face_border, const uint8_t* __restrict__ vert_border,
                                                    uint8_t* __restrict__ rejected) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int f = face[i];
    if (!icp_in_range(f, F)) {
        rejected[i] = 0;       // no face: not the border rule's business
        return;
    }
    const bool z[3] = {bary[i * 3 + 0] == 0.0f, bary[i * 3 + 1] == 0.0f, bary[i * 3 + 2] == 0.0f};
    const unsigned flags = face_border[f];
    bool out = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) out = out || (z[k] && ((flags >> k) & 1u));
    if ((int)z[0] + (int)z[1] + (int)z[2] == 2) {
        const int k = !z[0] ? 0 : (!z[1] ? 1 : 2);
        const int v = faces[(long long)f * 3 + k];
        out = out || (icp_in_range(v, V) && vert_border[v] != 0);
    }
    rejected[i] = out ? 1 : 0;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_ICP_COUNT(what, name, n) MOFA_REQUIRE((n) >= 1 && (n) <= kIcpMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

static int icp_inputs(const char* what, const float* moved, const float* target, const float* normals, const int32_t* face, const float* verts,
                      int64_t V, const int32_t* faces, int64_t F, const double* weight, int64_t N, const double pivot[3], int32_t metric,
                      IcpInputs& in) {
    MOFA_REQUIRE(moved && target && weight && pivot, "%s: null pointer", what);
    MOFA_REQUIRE(N >= 1 && N <= kIcpMaxIndex, "%s: N = %lld (want 1 .. 2^31 - 1)", what, (long long)N);
    MOFA_REQUIRE(metric == MOFA_ICP_POINT || metric == MOFA_ICP_PLANE, "%s: metric = %d (want MOFA_ICP_POINT or MOFA_ICP_PLANE)", what, (int)metric);
    if (metric == MOFA_ICP_PLANE) {
        MOFA_REQUIRE((face != nullptr) != (normals != nullptr), "%s: the plane metric takes the closest faces or explicit normals, one of the two", what);
        if (face) {
            MOFA_REQUIRE(verts && faces, "%s: null mesh", what);
            MOFA_REQUIRE(V >= 1 && V <= kIcpMaxIndex && F >= 1 && F <= kIcpMaxIndex, "%s: V = %lld, F = %lld (want 1 .. 2^31 - 1)", what, (long long)V,
                         (long long)F);
        }
    }
    MOFA_REQUIRE(isfinite(pivot[0]) && isfinite(pivot[1]) && isfinite(pivot[2]), "%s: the pivot is not finite", what);
    in.moved = moved, in.target = target, in.normals = normals, in.face = face, in.verts = verts, in.faces = faces, in.weight = weight;
    in.N = N, in.V = V, in.F = F;
    in.mu[0] = pivot[0], in.mu[1] = pivot[1], in.mu[2] = pivot[2];
    return MOFA_OK;
}

extern "C" {

int mofa_icp_apply(const float* points, int64_t N, const double transform[13], float* out, void* stream) {
    MOFA_REQUIRE(points && transform && out, "icp_apply: null pointer");
    MOFA_ICP_COUNT("icp_apply", "N", N);
    IcpTransform T;
    T.s = transform[0];
    for (int k = 0; k < 9; ++k) T.R[k] = transform[1 + k];
    for (int k = 0; k < 3; ++k) T.t[k] = transform[10 + k];
    hipLaunchKernelGGL(k_icp_apply, dim3(blocks_of(N, 256)), dim3(256), 0, (hipStream_t)stream, points, (long long)N, T, out);
    return check_launch("k_icp_apply");
}

int mofa_icp_terms(const float* moved, const float* target, const float* normals, const int32_t* face, const float* verts, int64_t V,
                   const int32_t* faces, int64_t F, const double* weight, int64_t N, const double pivot[3], int32_t metric, double* terms,
                   void* stream) {
    IcpInputs in;
    if (int rc = icp_inputs("icp_terms", moved, target, normals, face, verts, V, faces, F, weight, N, pivot, metric, in)) return rc;
    MOFA_REQUIRE(terms, "icp_terms: null pointer");
    if (metric == MOFA_ICP_PLANE)
        hipLaunchKernelGGL(k_icp_terms<1>, dim3(blocks_of(N, 256)), dim3(256), 0, (hipStream_t)stream, in, terms);
    else
        hipLaunchKernelGGL(k_icp_terms<0>, dim3(blocks_of(N, 256)), dim3(256), 0, (hipStream_t)stream, in, terms);
    return check_launch("k_icp_terms");
}

int mofa_icp_terms_reduce(const float* moved, const float* target, const float* normals, const int32_t* face, const float* verts, int64_t V,
                          const int32_t* faces, int64_t F, const double* weight, int64_t N, const double pivot[3], int32_t metric,
                          double* partial, void* stream) {
    IcpInputs in;
    if (int rc = icp_inputs("icp_terms_reduce", moved, target, normals, face, verts, V, faces, F, weight, N, pivot, metric, in)) return rc;
    MOFA_REQUIRE(partial, "icp_terms_reduce: null pointer");
    if (metric == MOFA_ICP_PLANE)
        hipLaunchKernelGGL(k_icp_terms_reduce<1>, dim3(blocks_of(N, kIcpChunk)), dim3(256), 0, (hipStream_t)stream, in, partial);
    else
        hipLaunchKernelGGL(k_icp_terms_reduce<0>, dim3(blocks_of(N, kIcpChunk)), dim3(256), 0, (hipStream_t)stream, in, partial);
    return check_launch("k_icp_terms_reduce");
}

int mofa_icp_reduce(const double* in, int64_t M, int32_t ncols, double* out, void* stream) {
    MOFA_REQUIRE(in && out, "icp_reduce: null pointer");
    MOFA_REQUIRE(in != out, "icp_reduce: the reduction does not run in place (in == out)");
    MOFA_ICP_COUNT("icp_reduce", "M", M);
    MOFA_REQUIRE(ncols >= 1 && ncols <= kIcpCols, "icp_reduce: ncols = %d (want 1 .. %d)", (int)ncols, kIcpCols);
    hipLaunchKernelGGL(k_icp_reduce, dim3(blocks_of(M, kIcpChunk)), dim3(256), 0, (hipStream_t)stream, in, (long long)M, (int)ncols, out);
    return check_launch("k_icp_reduce");
}

int mofa_icp_reject(const int32_t* face, const float* bary, int64_t N, const int32_t* faces, int64_t F, int64_t V, const uint8_t* face_border,
                    const uint8_t* vert_border, uint8_t* rejected, void* stream) {
    MOFA_REQUIRE(face && bary && faces && face_border && vert_border && rejected, "icp_reject: null pointer");
    MOFA_ICP_COUNT("icp_reject", "N", N);
    MOFA_ICP_COUNT("icp_reject", "F", F);
    MOFA_ICP_COUNT("icp_reject", "V", V);
    hipLaunchKernelGGL(k_icp_reject, dim3(blocks_of(N, 256)), dim3(256), 0, (hipStream_t)stream, face, bary, (long long)N, faces, (long long)F,
                       (long long)V, face_border, vert_border, rejected);
    return check_launch("k_icp_reject");
}

}  // extern "C"
