// UV texture baking for the geometry export (gfx950): the map between the texels of a texture image and the surface of a mesh with an
// OBJ-style per-corner UV layout (uvs [T,2] float, uv_faces [F,3] int32), and the image-side operations around mofa_bake_integrate.
// mesh.py drives the passes (mesh.uv_locate / texel_map / texel_surface / dilate_texture / sample_texture).  One thread per element, all
// arithmetic fp64 on the fp32 inputs widened, every operation rounded separately (the build pins -ffp-contract=off); no float or double
// atomic exists (the only atomics are the integer counters, one per wavefront); every index is checked before it is dereferenced: a bad
// one is skipped and counted, never a fault; nothing waits on another thread.
//
// A texture is [Ht,Wt,C] float, row 0 at the top: texel (i, j) has its centre at u = (j + 0.5) / Wt, v = 1 - (i + 0.5) / Ht, and a UV
// maps to the continuous texel coordinates x = u Wt - 0.5, y = (1 - v) Ht - 0.5.  No wrap-around.
//
//   locate    query q against face f with UV corners A, B, C:   D = (B.u - A.u) (C.v - A.v) - (B.v - A.v) (C.u - A.u);  D == 0 or not
//             finite: skipped.  Edge k is the one opposite corner k (B -> C, C -> A, A -> B).  Of its two endpoints P is the
//             lexicographically smaller (u, then v) and Q the other:   E = (Q.u - P.u) (q.v - P.v) - (Q.v - P.v) (q.u - P.u),
//             negated where the face runs the edge from Q to P, and negated again when D < 0 (a mirrored chart): e_k.  Two faces that
//             share an edge, by index or (across a seam) by coordinates, compute the same bits up to an exact sign.
//             inside: e_0 >= 0, e_1 >= 0, e_2 >= 0 and S = (e_0 + e_1) + e_2 > 0;  bary_k = e_k / S;  the lowest containing face wins
//             strictly inside (all e_k > 0) two or more faces: counted in MULTI
//   surface   point[a] = (float)((b0 X0[a] + b1 X1[a]) + b2 X2[a]);  normal: m = the same interpolation of the vertex normals, or
//             (X1 - X0) x (X2 - X0);  len = sqrt((m.x m.x + m.y m.y) + m.z m.z);  (float)(m / len), (0, 0, 0) unless len > 0 and finite
//   dilate    an invalid texel with k >= 1 valid texels among its 8 neighbours inside the image: (float)(s / k), s the fp64 sum of their
//             INPUT colours in row-major order of the 3 x 3 window, and valid;  every other texel copied
//   sample    u = (b0 u0 + b1 u1) + b2 u2, v likewise (never rounded to float);  x, y as above;  j0 = floor(x), fx = x - j0, i0 =
//             floor(y), fy = y - i0;  j0, j0 + 1, i0, i0 + 1 clamped to the image;  a = c00 + fx (c10 - c00), b = c01 + fx (c11 - c01),
//             (float)(a + fy (b - a))  (mofa_bake_integrate's order; c10 is the texel at (i0, j0 + 1))
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kUvMaxIndex = (1ll << 31) - 1;       // N, T, V, F, the pair count, the texels of an image: int32 indices
constexpr int kUvMaxChannels = 16;

struct UvGrid {
    double origin[2], cell[2];
    int n[2];
};

__device__ __forceinline__ bool uv_in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

// mofa_wind_bin_*'s cell index (the lists this file walks are theirs)
__device__ __forceinline__ int uv_cell(double x, double origin, double cell, int n) {
    const double t = floor((x - origin) / cell);
    return t >= 0.0 ? (t < (double)n ? (int)t : n - 1) : 0;          // (NaN: 0)
}

// sums `v` over the wavefront (every lane of it must call) and adds the total to counts[slot]: one integer atomic per wavefront
__device__ __forceinline__ void uv_wave_add(int64_t* counts, int slot, unsigned long long v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w);
    if (__lane_id() == 0 && v) atomicAdd((unsigned long long*)(counts + slot), v);
}

// the edge function of q against the edge the face runs from X to Y, on the edge's endpoints in coordinate order
__device__ __forceinline__ double uv_edge(double xu, double xv, double yu, double yv, double qu, double qv, bool mirrored) {
    const bool from_q = yu < xu || (yu == xu && yv < xv);             // Y is the smaller endpoint: the face runs Q -> P
    const double pu = from_q ? yu : xu, pv = from_q ? yv : xv, su = from_q ? xu : yu, sv = from_q ? xv : yv;
    const double e = (su - pu) * (qv - pv) - (sv - pv) * (qu - pu);
    return from_q != mirrored ? -e : e;
}

__device__ __forceinline__ double uv_det(double au, double av, double bu, double bv, double cu, double cv) {
    return (bu - au) * (cv - av) - (bv - av) * (cu - au);
}

// counts[MOFA_UV_DEGENERATE] += the faces whose D is 0 or not finite (a face with an index outside [0, T) is passed over)
__global__ __launch_bounds__(256) void k_uv_degenerate(const float* __restrict__ uvs, int T, const int* __restrict__ uv_faces, long long F,
                                                       int64_t* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool degenerate = false;
    if (f < F) {
        const int t0 = uv_faces[f * 3 + 0], t1 = uv_faces[f * 3 + 1], t2 = uv_faces[f * 3 + 2];
        if (uv_in_range(t0, T) && uv_in_range(t1, T) && uv_in_range(t2, T)) {
            const double d = uv_det((double)uvs[(long long)t0 * 2], (double)uvs[(long long)t0 * 2 + 1], (double)uvs[(long long)t1 * 2],
                                    (double)uvs[(long long)t1 * 2 + 1], (double)uvs[(long long)t2 * 2], (double)uvs[(long long)t2 * 2 + 1]);
            degenerate = !isfinite(d) || d == 0.0;
        }
    }
    uv_wave_add(counts, MOFA_UV_DEGENERATE, degenerate ? 1ull : 0ull);
}

__global__ __launch_bounds__(256) void k_uv_locate(const double* __restrict__ queries, long long N, const int64_t* __restrict__ order,
                                                   const float* __restrict__ uvs, int T, const int* __restrict__ uv_faces, int F,
                                                   const int* __restrict__ cell_start, const int* __restrict__ pair_face, int P, UvGrid g,
                                                   int* __restrict__ face, double* __restrict__ bary, int64_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long q = -1;
    if (i < N) {
        q = order ? order[i] : i;
        if (q < 0 || q >= N) q = -1;
    }
    unsigned long long tests = 0;
    bool non_finite = false, multi = false;
    if (q >= 0) {
        const double qu = queries[q * 2 + 0], qv = queries[q * 2 + 1];
        non_finite = !(isfinite(qu) && isfinite(qv));
        int best = -1, strict = 0;
        double b0 = NAN, b1 = NAN, b2 = NAN;
        if (!non_finite && P > 0) {
            const int col = uv_cell(qu, g.origin[0], g.cell[0], g.n[0]) * g.n[1] + uv_cell(qv, g.origin[1], g.cell[1], g.n[1]);
            int j0 = cell_start[col], j1 = cell_start[col + 1];
            j0 = j0 < 0 ? 0 : j0, j1 = j1 > P ? P : j1;
            for (int j = j0; j < j1; ++j) {
                const int f = pair_face[j];
                if (!uv_in_range(f, F)) continue;
                const int t0 = uv_faces[(long long)f * 3 + 0], t1 = uv_faces[(long long)f * 3 + 1], t2 = uv_faces[(long long)f * 3 + 2];
                if (!uv_in_range(t0, T) || !uv_in_range(t1, T) || !uv_in_range(t2, T)) continue;
                const double au = (double)uvs[(long long)t0 * 2], av = (double)uvs[(long long)t0 * 2 + 1];
                const double bu = (double)uvs[(long long)t1 * 2], bv = (double)uvs[(long long)t1 * 2 + 1];
                const double cu = (double)uvs[(long long)t2 * 2], cv = (double)uvs[(long long)t2 * 2 + 1];
                ++tests;
                const double d = uv_det(au, av, bu, bv, cu, cv);
                if (!isfinite(d) || d == 0.0) continue;
                const bool mirrored = d < 0.0;
                const double e0 = uv_edge(bu, bv, cu, cv, qu, qv, mirrored), e1 = uv_edge(cu, cv, au, av, qu, qv, mirrored),
                             e2 = uv_edge(au, av, bu, bv, qu, qv, mirrored);
                if (!(e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0)) continue;
                const double s = (e0 + e1) + e2;
                if (!(s > 0.0)) continue;
                if (e0 > 0.0 && e1 > 0.0 && e2 > 0.0) ++strict;
                if (best < 0 || f < best) best = f, b0 = e0 / s, b1 = e1 / s, b2 = e2 / s;
            }
        }
        face[q] = best;
        bary[q * 3 + 0] = b0, bary[q * 3 + 1] = b1, bary[q * 3 + 2] = b2;
        multi = strict >= 2;
    }
    uv_wave_add(counts, MOFA_UV_NON_FINITE, non_finite ? 1ull : 0ull);
    uv_wave_add(counts, MOFA_UV_TESTS, tests);
    uv_wave_add(counts, MOFA_UV_MULTI, multi ? 1ull : 0ull);
}

__global__ __launch_bounds__(256) void k_uv_surface(const int* __restrict__ face, const double* __restrict__ bary, long long N,
                                                    const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                    const float* __restrict__ normals, float* __restrict__ points,
                                                    float* __restrict__ normals_out, int64_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool skipped = false;
    if (i < N) {
        const int f = face[i];
        int i0 = -1, i1 = -1, i2 = -1;
        if (uv_in_range(f, F)) i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
        skipped = !(uv_in_range(i0, V) && uv_in_range(i1, V) && uv_in_range(i2, V));
        if (skipped) {
#pragma unroll
            for (int a = 0; a < 3; ++a) points[i * 3 + a] = NAN, normals_out[i * 3 + a] = 0.0f;
        } else {
            const double b0 = bary[i * 3 + 0], b1 = bary[i * 3 + 1], b2 = bary[i * 3 + 2];
            const double x0[3] = {(double)verts[(long long)i0 * 3], (double)verts[(long long)i0 * 3 + 1], (double)verts[(long long)i0 * 3 + 2]};
            const double x1[3] = {(double)verts[(long long)i1 * 3], (double)verts[(long long)i1 * 3 + 1], (double)verts[(long long)i1 * 3 + 2]};
            const double x2[3] = {(double)verts[(long long)i2 * 3], (double)verts[(long long)i2 * 3 + 1], (double)verts[(long long)i2 * 3 + 2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) points[i * 3 + a] = (float)((b0 * x0[a] + b1 * x1[a]) + b2 * x2[a]);
            double m[3];
            if (normals) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    m[a] = (b0 * (double)normals[(long long)i0 * 3 + a] + b1 * (double)normals[(long long)i1 * 3 + a]) +
                           b2 * (double)normals[(long long)i2 * 3 + a];
            } else {
                const double p[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, r[3] = {x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2]};
                m[0] = p[1] * r[2] - p[2] * r[1], m[1] = p[2] * r[0] - p[0] * r[2], m[2] = p[0] * r[1] - p[1] * r[0];
            }
            const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            const bool ok = len > 0.0 && isfinite(len);
#pragma unroll
            for (int a = 0; a < 3; ++a) normals_out[i * 3 + a] = ok ? (float)(m[a] / len) : 0.0f;
        }
    }
    uv_wave_add(counts, 0, skipped ? 1ull : 0ull);
}

// one gutter-filling step: reads `in` / `vin` only, writes `out` / `vout` only
__global__ __launch_bounds__(256) void k_uv_dilate(int Ht, int Wt, int C, const float* __restrict__ in, const uint8_t* __restrict__ vin,
                                                   float* __restrict__ out, uint8_t* __restrict__ vout) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)Ht * Wt) return;
    const int i = (int)(t / Wt), j = (int)(t - (long long)i * Wt);
    int k = 0;
    if (!vin[t]) {
        for (int di = -1; di <= 1; ++di)
            for (int dj = -1; dj <= 1; ++dj) {
                const int a = i + di, b = j + dj;
                if ((di || dj) && a >= 0 && a < Ht && b >= 0 && b < Wt && vin[(long long)a * Wt + b]) ++k;
            }
    }
    if (k == 0) {
        for (int ch = 0; ch < C; ++ch) out[t * C + ch] = in[t * C + ch];
        vout[t] = vin[t];
        return;
    }
    for (int ch = 0; ch < C; ++ch) {
        double s = 0.0;
        for (int di = -1; di <= 1; ++di)
            for (int dj = -1; dj <= 1; ++dj) {
                const int a = i + di, b = j + dj;
                if ((di || dj) && a >= 0 && a < Ht && b >= 0 && b < Wt && vin[(long long)a * Wt + b])
                    s = s + (double)in[((long long)a * Wt + b) * C + ch];
            }
        out[t * C + ch] = (float)(s / (double)k);
    }
    vout[t] = 1;
}

// a texel index of the continuous coordinate's floor `f` (+ 0 or 1), clamped to [0, n - 1] on the double
__device__ __forceinline__ int uv_clamp(double f, int n) { return f >= 0.0 ? (f <= (double)(n - 1) ? (int)f : n - 1) : 0; }

__global__ __launch_bounds__(256) void k_uv_sample(const int* __restrict__ face, const float* __restrict__ bary, long long N,
                                                   const float* __restrict__ uvs, int T, const int* __restrict__ uv_faces, int F,
                                                   const float* __restrict__ texture, int Ht, int Wt, int C, float background,
                                                   float* __restrict__ out, int64_t* __restrict__ counts) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    bool empty = false;
    if (p < N) {
        const int f = face[p];
        int t0 = -1, t1 = -1, t2 = -1;
        if (uv_in_range(f, F)) t0 = uv_faces[(long long)f * 3 + 0], t1 = uv_faces[(long long)f * 3 + 1], t2 = uv_faces[(long long)f * 3 + 2];
        double u = NAN, v = NAN;
        if (uv_in_range(t0, T) && uv_in_range(t1, T) && uv_in_range(t2, T)) {
            const double b0 = (double)bary[p * 3 + 0], b1 = (double)bary[p * 3 + 1], b2 = (double)bary[p * 3 + 2];
            u = (b0 * (double)uvs[(long long)t0 * 2] + b1 * (double)uvs[(long long)t1 * 2]) + b2 * (double)uvs[(long long)t2 * 2];
            v = (b0 * (double)uvs[(long long)t0 * 2 + 1] + b1 * (double)uvs[(long long)t1 * 2 + 1]) + b2 * (double)uvs[(long long)t2 * 2 + 1];
        }
        empty = !(isfinite(u) && isfinite(v));
        if (empty) {
            for (int ch = 0; ch < C; ++ch) out[p * C + ch] = background;
        } else {
            const double x = u * (double)Wt - 0.5, y = (1.0 - v) * (double)Ht - 0.5;
            const double xf = floor(x), yf = floor(y);
            const double fx = x - xf, fy = y - yf;
            const long long j0 = uv_clamp(xf, Wt), j1 = uv_clamp(xf + 1.0, Wt), i0 = uv_clamp(yf, Ht), i1 = uv_clamp(yf + 1.0, Ht);
            const long long o00 = (i0 * Wt + j0) * C, o10 = (i0 * Wt + j1) * C, o01 = (i1 * Wt + j0) * C, o11 = (i1 * Wt + j1) * C;
            for (int ch = 0; ch < C; ++ch) {
                const double c00 = (double)texture[o00 + ch], c10 = (double)texture[o10 + ch], c01 = (double)texture[o01 + ch],
                             c11 = (double)texture[o11 + ch];
                const double a = c00 + fx * (c10 - c00);
                const double b = c01 + fx * (c11 - c01);
                out[p * C + ch] = (float)(a + fy * (b - a));
            }
        }
    }
    uv_wave_add(counts, 0, empty ? 1ull : 0ull);
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

bool uv_grid(const double* origin, const double* cell, const int32_t* n, UvGrid& g) {
    for (int a = 0; a < 2; ++a) {
        g.origin[a] = origin[a], g.cell[a] = cell[a], g.n[a] = n[a];
        if (!isfinite(origin[a]) || !isfinite(cell[a]) || !(cell[a] > 0.0)) return false;
        if (n[a] < 1 || n[a] > MOFA_WIND_MAX_GRID) return false;
    }
    return true;                                                 // (at most 4096^2 cells: they fit an int32)
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_UV_COUNT(what, name, n) MOFA_REQUIRE((n) >= 1 && (n) <= kUvMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))
#define MOFA_UV_IMAGE(what)                                                                                                                  \
    MOFA_REQUIRE(Ht >= 1 && Wt >= 1 && (long long)Ht * Wt <= kUvMaxIndex, what ": Ht = %d, Wt = %d (want Ht, Wt >= 1 and Ht Wt < 2^31)", (int)Ht, \
                 (int)Wt);                                                                                                                   \
    MOFA_REQUIRE(C >= 1 && C <= kUvMaxChannels, what ": C = %d channels (want 1 .. %d)", (int)C, kUvMaxChannels)

extern "C" {

int mofa_uv_locate(const double* queries, int64_t N, const int64_t* order, const float* uvs, int64_t T, const int32_t* uv_faces, int64_t F,
                   const double origin[2], const double cell[2], const int32_t n[2], const int32_t* cell_start, const int32_t* pair_face, int64_t P,
                   int32_t* face, double* bary, int64_t* counts, void* stream) {
    MOFA_REQUIRE(queries && uvs && uv_faces && origin && cell && n && cell_start && face && bary && counts, "uv_locate: null pointer");
    MOFA_UV_COUNT("uv_locate", "N", N);
    MOFA_UV_COUNT("uv_locate", "T", T);
    MOFA_UV_COUNT("uv_locate", "F", F);
    MOFA_REQUIRE(P >= 0 && P <= kUvMaxIndex && (pair_face || P == 0), "uv_locate: P = %lld (want 0 .. 2^31 - 1, and the pairs unless it is 0)",
                 (long long)P);
    UvGrid g;
    MOFA_REQUIRE(uv_grid(origin, cell, n, g), "uv_locate: origin / cell must be finite, cell > 0, 1 <= n <= 4096 per axis");
    hipLaunchKernelGGL(k_uv_degenerate, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, uvs, (int)T, uv_faces, (long long)F, counts);
    if (int rc = check_launch("k_uv_degenerate")) return rc;
    hipLaunchKernelGGL(k_uv_locate, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, queries, (long long)N, order, uvs, (int)T, uv_faces,
                       (int)F, cell_start, pair_face, (int)P, g, face, bary, counts);
    return check_launch("k_uv_locate");
}

int mofa_uv_surface(const int32_t* face, const double* bary, int64_t N, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                    const float* normals, float* points, float* normals_out, int64_t* counts, void* stream) {
    MOFA_REQUIRE(face && bary && verts && faces && points && normals_out && counts, "uv_surface: null pointer");
    MOFA_UV_COUNT("uv_surface", "N", N);
    MOFA_UV_COUNT("uv_surface", "V", V);
    MOFA_UV_COUNT("uv_surface", "F", F);
    hipLaunchKernelGGL(k_uv_surface, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, face, bary, (long long)N, verts, (int)V, faces, (int)F,
                       normals, points, normals_out, counts);
    return check_launch("k_uv_surface");
}

int mofa_uv_dilate(const float* texture_in, const uint8_t* valid_in, int32_t Ht, int32_t Wt, int32_t C, float* texture_out, uint8_t* valid_out,
                   void* stream) {
    MOFA_REQUIRE(texture_in && valid_in && texture_out && valid_out, "uv_dilate: null pointer");
    MOFA_UV_IMAGE("uv_dilate");
    MOFA_REQUIRE(texture_in != texture_out && valid_in != valid_out, "uv_dilate: the step is double-buffered (input and output must differ)");
    hipLaunchKernelGGL(k_uv_dilate, dim3(blocks_of((long long)Ht * Wt)), dim3(256), 0, (hipStream_t)stream, (int)Ht, (int)Wt, (int)C, texture_in,
                       valid_in, texture_out, valid_out);
    return check_launch("k_uv_dilate");
}

int mofa_uv_sample(const int32_t* face, const float* bary, int64_t N, const float* uvs, int64_t T, const int32_t* uv_faces, int64_t F,
                   const float* texture, int32_t Ht, int32_t Wt, int32_t C, float background, float* out, int64_t* counts, void* stream) {
    MOFA_REQUIRE(face && bary && uvs && uv_faces && texture && out && counts, "uv_sample: null pointer");
    MOFA_UV_COUNT("uv_sample", "N", N);
    MOFA_UV_COUNT("uv_sample", "T", T);
    MOFA_UV_COUNT("uv_sample", "F", F);
    MOFA_UV_IMAGE("uv_sample");
    hipLaunchKernelGGL(k_uv_sample, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, face, bary, (long long)N, uvs, (int)T, uv_faces, (int)F,
                       texture, (int)Ht, (int)Wt, (int)C, background, out, counts);
    return check_launch("k_uv_sample");
}

}  // extern "C"
