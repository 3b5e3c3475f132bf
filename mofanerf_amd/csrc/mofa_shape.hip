// Linear shape models for the geometry export (gfx950): the device side of mesh.shape_model / shape_synthesize / shape_project / shape_fit.
// mesh.py drives everything: the decomposition of the M x M Gram matrix (cyclic Jacobi) and the K x K solves (Cholesky) run on the host.
// Nothing here waits on another thread and there is no atomic of any kind: every sum has a fixed order that does not depend on the launch
// geometry or on how the pairs are tiled, so the same input gives the same bytes.  All arithmetic is fp64, every operation rounded
// separately (the build pins -ffp-contract=off); no matrix instruction is used (the fp64 ones fuse the multiply and the add).  The order of
// operations is the header's (include/mofanerf_hip.h); in short:
//
//   gram     partial[k][pair(a, b)] = the sum over chunk k = columns [1024 k, 1024 (k + 1)) of  term_j = w[j / group] * (P[a][j] * P[b][j])
//            (no weights: P[a][j] * P[b][j]; `w > 0` false: the column adds nothing, whatever P holds):  thread t of 256 starts from 0.0
//            and adds the columns t, t + 256, t + 512, t + 768 in that order, then the tree `for w = 128 .. 1: p[t] += p[t + w] (t < w)`.
//            pair(a, b), a <= b: the upper triangle row by row.  A workgroup owns one chunk and one 8 x 8 tile of pairs; a thread keeps the
//            64 sums of its columns in registers (8 + 8 loads per column) and the tree runs 8 pairs at a time through the LDS.
//   reduce   mofa_icp_reduce's sum for rows of any width: out[k][c] from in[1024 k .. 1024 (k + 1))[c], the same additions in the same order.
//   centre   mean[j] = (0.0 + meshes[0][j] + meshes[1][j] + ..) / M;   X[m][j] = meshes[m][j] - mean[j]
//   combine  acc = 0.0;  acc += coef[b][r] * rows[r][j]  (r ascending);  out[b][j] = base ? base[j] + acc : acc
//   rows     n = the unit normal of the closest face (icp_row<PLANE>'s);  q_c = s * ((R[0][c] n_x + R[1][c] n_y) + R[2][c] n_z);
//            P[k][i] = (q_x m_kx + q_y m_ky) + q_z m_kz;   P[K][i] = (n_x d_x + n_y d_y) + n_z d_z,  d = moved - closest
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kShapeMaxIndex = (1ll << 31) - 1;
constexpr int kShapeChunk = MOFA_ICP_CHUNK;             // 1024 columns per workgroup: 4 per thread, a fixed trip count
constexpr int kShapeTile = 8;                           // pairs per workgroup: 8 x 8
constexpr int kShapeRedCols = 16;                       // columns of a wide row one workgroup of the reduce owns

__device__ __forceinline__ bool shape_in_range(int v, long long n) { return v >= 0 && (long long)v < n; }

// 64 accumulators + 16 operands in fp64 and the addresses: 200 VGPRs without weights, 204 with (the code object's figures): two waves per
// SIMD (the file holds 512 per lane), no scratch
template <int WEIGHTED>
__global__ __launch_bounds__(256) void k_shape_gram(const double* __restrict__ P, int R, long long N, const double* __restrict__ weight, int group,
                                                    int tiles, double* __restrict__ partial) {
    __shared__ double sm[kShapeTile][256];
    // blockIdx.y counts the tile pairs (ta <= tb) row by row
    int ta = 0, rest = (int)blockIdx.y;
    while (rest >= tiles - ta) {
        rest -= tiles - ta;
        ++ta;
    }
    const int tb = ta + rest;
    const int a0 = ta * kShapeTile, b0 = tb * kShapeTile;
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * kShapeChunk;
    double acc[kShapeTile][kShapeTile];
#pragma unroll
    for (int i = 0; i < kShapeTile; ++i)
#pragma unroll
        for (int j = 0; j < kShapeTile; ++j) acc[i][j] = 0.0;
#pragma unroll 1
    for (int k = 0; k < kShapeChunk / 256; ++k) {
        const long long col = c0 + t + (long long)k * 256;
        if (col >= N) continue;
        double w = 1.0;
        if (WEIGHTED) {
            w = weight[col / group];
            if (!(w > 0.0)) continue;
        }
        double pa[kShapeTile], pb[kShapeTile];
#pragma unroll
        for (int i = 0; i < kShapeTile; ++i) {
            pa[i] = a0 + i < R ? P[(long long)(a0 + i) * N + col] : 0.0;
            pb[i] = b0 + i < R ? P[(long long)(b0 + i) * N + col] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < kShapeTile; ++i)
#pragma unroll
            for (int j = 0; j < kShapeTile; ++j) {
                const double prod = pa[i] * pb[j];
                acc[i][j] += WEIGHTED ? w * prod : prod;
            }
    }
    const long long npairs = (long long)R * (R + 1) / 2;
    double* __restrict__ out_row = partial + (long long)blockIdx.x * npairs;
#pragma unroll
    for (int i = 0; i < kShapeTile; ++i) {
#pragma unroll
        for (int j = 0; j < kShapeTile; ++j) sm[j][t] = acc[i][j];
        __syncthreads();
#pragma unroll
        for (int w = 128; w >= 1; w >>= 1) {
            if (t < w) {
#pragma unroll
                for (int j = 0; j < kShapeTile; ++j) sm[j][t] += sm[j][t + w];
            }
            __syncthreads();
        }
        const int a = a0 + i, b = b0 + t;
        if (t < kShapeTile && a < R && b < R && a <= b) out_row[(long long)a * R - (long long)a * (a - 1) / 2 + (b - a)] = sm[t][0];
        __syncthreads();
    }
}

// thread (lane l = t / 16, column c = t % 16): the partial sums p_u of u = l, l + 16, .. of its column, then its share of the tree
__global__ __launch_bounds__(256) void k_shape_reduce(const double* __restrict__ in, long long M, long long ncols, double* __restrict__ out) {
    __shared__ double sm[256][kShapeRedCols];
    const int c = threadIdx.x % kShapeRedCols, l = threadIdx.x / kShapeRedCols;
    constexpr int kLanes = 256 / kShapeRedCols;
    const long long col = (long long)blockIdx.y * kShapeRedCols + c;
    const long long r0 = (long long)blockIdx.x * kShapeChunk;
    const bool live = col < ncols;
    for (int u = l; u < 256; u += kLanes) {
        double p = 0.0;
#pragma unroll
        for (int k = 0; k < kShapeChunk / 256; ++k) {
            const long long row = r0 + u + (long long)k * 256;
            if (live && row < M) p += in[row * ncols + col];
        }
        sm[u][c] = p;
    }
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        for (int u = l; u < w; u += kLanes) sm[u][c] += sm[u + w][c];
        __syncthreads();
    }
    if (l == 0 && live) out[(long long)blockIdx.x * ncols + col] = sm[0][c];
}

__global__ __launch_bounds__(256) void k_shape_centre(const float* __restrict__ meshes, int M, long long n, double* __restrict__ mean,
                                                      double* __restrict__ X) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += (double)meshes[(long long)m * n + j];
    const double mu = s / (double)M;
    mean[j] = mu;
    for (int m = 0; m < M; ++m) X[(long long)m * n + j] = (double)meshes[(long long)m * n + j] - mu;
}

__global__ __launch_bounds__(256) void k_shape_combine(const double* __restrict__ base, const double* __restrict__ coef, const double* __restrict__ rows,
                                                       int R, long long n, double* __restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long long b = blockIdx.y;
    double acc = 0.0;
    for (int r = 0; r < R; ++r) acc += coef[b * R + r] * rows[(long long)r * n + j];
    out[b * n + j] = base ? base[j] + acc : acc;
}

struct ShapePose {
    double s, R[9];
};

__global__ __launch_bounds__(256) void k_shape_plane_rows(const float* __restrict__ moved, const float* __restrict__ closest,
                                                          const int* __restrict__ face, const float* __restrict__ verts, long long TV,
                                                          const int* __restrict__ faces, long long TF, ShapePose T, const double* __restrict__ modes,
                                                          int K, long long V, double* __restrict__ P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const double nan = __builtin_nan("");
    bool ok = false;
    double n[3] = {nan, nan, nan};
    const int f = face[i];
    if (shape_in_range(f, TF)) {
        const int ia = faces[(long long)f * 3 + 0], ib = faces[(long long)f * 3 + 1], ic = faces[(long long)f * 3 + 2];
        if (shape_in_range(ia, TV) && shape_in_range(ib, TV) && shape_in_range(ic, TV)) {
            double a[3], ab[3], ac[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a[k] = (double)verts[(long long)ia * 3 + k];
                ab[k] = (double)verts[(long long)ib * 3 + k] - a[k];
                ac[k] = (double)verts[(long long)ic * 3 + k] - a[k];
            }
            const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
            const double len = sqrt((cx * cx + cy * cy) + cz * cz);
            n[0] = cx / len, n[1] = cy / len, n[2] = cz / len;
            ok = true;
        }
    }
    if (!ok) {
        for (int k = 0; k <= K; ++k) P[(long long)k * V + i] = nan;
        return;
    }
    double q[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[c] = T.s * ((T.R[0 * 3 + c] * n[0] + T.R[1 * 3 + c] * n[1]) + T.R[2 * 3 + c] * n[2]);
        d[c] = (double)moved[i * 3 + c] - (double)closest[i * 3 + c];
    }
    for (int k = 0; k < K; ++k) {
        const double* __restrict__ m = modes + ((long long)k * V + i) * 3;
        P[(long long)k * V + i] = (q[0] * m[0] + q[1] * m[1]) + q[2] * m[2];
    }
    P[(long long)K * V + i] = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
}

inline unsigned shape_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_SHAPE_COUNT(what, name, n) MOFA_REQUIRE((n) >= 1 && (n) <= kShapeMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

extern "C" {

int mofa_shape_gram(const double* P, int32_t R, int64_t N, const double* weight, int32_t group, double* partial, void* stream) {
    MOFA_REQUIRE(P && partial, "shape_gram: null pointer");
    MOFA_REQUIRE(R >= 1 && R <= MOFA_SHAPE_MAX_ROWS, "shape_gram: R = %d (want 1 .. %d)", (int)R, MOFA_SHAPE_MAX_ROWS);
    MOFA_SHAPE_COUNT("shape_gram", "N", N);
    MOFA_REQUIRE(group == 1 || group == 3, "shape_gram: group = %d (want 1 or 3)", (int)group);
    MOFA_REQUIRE(!weight || N % group == 0, "shape_gram: N = %lld is no multiple of group = %d", (long long)N, (int)group);
    const int tiles = (R + kShapeTile - 1) / kShapeTile;
    const dim3 grid(shape_blocks(N, kShapeChunk), (unsigned)(tiles * (tiles + 1) / 2));
    if (weight)
        hipLaunchKernelGGL(k_shape_gram<1>, grid, dim3(256), 0, (hipStream_t)stream, P, (int)R, (long long)N, weight, (int)group, tiles, partial);
    else
        hipLaunchKernelGGL(k_shape_gram<0>, grid, dim3(256), 0, (hipStream_t)stream, P, (int)R, (long long)N, weight, 1, tiles, partial);
    return check_launch("k_shape_gram");
}

int mofa_shape_reduce(const double* in, int64_t M, int64_t ncols, double* out, void* stream) {
    MOFA_REQUIRE(in && out, "shape_reduce: null pointer");
    MOFA_REQUIRE(in != out, "shape_reduce: the reduction does not run in place (in == out)");
    MOFA_SHAPE_COUNT("shape_reduce", "M", M);
    MOFA_REQUIRE(ncols >= 1 && ncols <= (int64_t)MOFA_SHAPE_MAX_ROWS * (MOFA_SHAPE_MAX_ROWS + 1) / 2, "shape_reduce: ncols = %lld (want 1 .. %d)",
                 (long long)ncols, MOFA_SHAPE_MAX_ROWS * (MOFA_SHAPE_MAX_ROWS + 1) / 2);
    const dim3 grid(shape_blocks(M, kShapeChunk), shape_blocks(ncols, kShapeRedCols));
    hipLaunchKernelGGL(k_shape_reduce, grid, dim3(256), 0, (hipStream_t)stream, in, (long long)M, (long long)ncols, out);
    return check_launch("k_shape_reduce");
}

int mofa_shape_centre(const float* meshes, int32_t M, int64_t n, double* mean, double* X, void* stream) {
    MOFA_REQUIRE(meshes && mean && X, "shape_centre: null pointer");
    MOFA_REQUIRE(M >= 1 && M <= MOFA_SHAPE_MAX_ROWS, "shape_centre: M = %d (want 1 .. %d)", (int)M, MOFA_SHAPE_MAX_ROWS);
    MOFA_SHAPE_COUNT("shape_centre", "n", n);
    hipLaunchKernelGGL(k_shape_centre, dim3(shape_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, meshes, (int)M, (long long)n, mean, X);
    return check_launch("k_shape_centre");
}

int mofa_shape_combine(const double* base, const double* coef, const double* rows, int32_t B, int32_t R, int64_t n, double* out, void* stream) {
    MOFA_REQUIRE(coef && rows && out, "shape_combine: null pointer");
    MOFA_REQUIRE(B >= 1 && B <= 65535, "shape_combine: B = %d (want 1 .. 65535)", (int)B);
    MOFA_REQUIRE(R >= 1 && R <= MOFA_SHAPE_MAX_ROWS, "shape_combine: R = %d (want 1 .. %d)", (int)R, MOFA_SHAPE_MAX_ROWS);
    MOFA_SHAPE_COUNT("shape_combine", "n", n);
    MOFA_REQUIRE(out != rows && out != base, "shape_combine: the combination does not run in place");
    hipLaunchKernelGGL(k_shape_combine, dim3(shape_blocks(n, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, base, coef, rows, (int)R,
                       (long long)n, out);
    return check_launch("k_shape_combine");
}

int mofa_shape_plane_rows(const float* moved, const float* closest, const int32_t* face, const float* verts, int64_t TV, const int32_t* faces,
                          int64_t TF, const double transform[13], const double* modes, int32_t K, int64_t V, double* P, void* stream) {
    MOFA_REQUIRE(moved && closest && face && verts && faces && transform && P, "shape_plane_rows: null pointer");
    MOFA_REQUIRE(K >= 0 && K < MOFA_SHAPE_MAX_ROWS, "shape_plane_rows: K = %d (want 0 .. %d)", (int)K, MOFA_SHAPE_MAX_ROWS - 1);
    MOFA_REQUIRE(K == 0 || modes, "shape_plane_rows: null modes");
    MOFA_SHAPE_COUNT("shape_plane_rows", "V", V);
    MOFA_SHAPE_COUNT("shape_plane_rows", "TV", TV);
    MOFA_SHAPE_COUNT("shape_plane_rows", "TF", TF);
    ShapePose T;
    T.s = transform[0];
    for (int k = 0; k < 9; ++k) T.R[k] = transform[1 + k];
    hipLaunchKernelGGL(k_shape_plane_rows, dim3(shape_blocks(V, 256)), dim3(256), 0, (hipStream_t)stream, moved, closest, face, verts, (long long)TV,
                       faces, (long long)TF, T, modes, (int)K, (long long)V, P);
    return check_launch("k_shape_plane_rows");
}

}  // extern "C"
