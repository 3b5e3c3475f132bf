// Multi-view colour baking for the geometry export (gfx950): posed colour frames projected onto the vertices of a mesh with any
// triangulation, occlusion-aware through a depth frame per view, and the vertex colours made from what was gathered.  mesh.py drives the
// passes (mesh.bake_state / bake_integrate / bake_colors / fill_colors).  One thread per vertex; a vertex's state is read once, updated
// over the views of the call IN ORDER in registers and written once: no atomics, nothing waits on another thread, the same frames in the
// same order give the same bytes, and views [a | b] in two calls give the bytes of one call with a + b.  All arithmetic is fp64 on the fp32
// inputs widened, every operation rounded separately (the build pins -ffp-contract=off).  The camera of a view (16 floats) is read with a
// wave-uniform index, so it travels in scalar registers; the four depths and 4 C texels of the footprint are the only gathers, and their
// offsets are formed only after the footprint has been range-checked on the doubles.
//
//   integrate   vertex x, per view, c = its pose:
//                 d[a] = x[a] - c[a][3];  p[a] = (d0 c[0][a] + d1 c[1][a]) + d2 c[2][a];  t = -p[2]   (mofa_tsdf_integrate's projection)
//                 not t > 0: skip;  u = cx + fx (p0 / t), v = cy - fy (p1 / t);  u0 = floor(u), v0 = floor(v)
//                 unless 0 <= u0, u0 + 1 <= W - 1, 0 <= v0, v0 + 1 <= H - 1 (on the doubles: a non-finite value fails): skip
//                 D_k = depth at (v0, u0), (v0, u0 + 1), (v0 + 1, u0), (v0 + 1, u0 + 1);  any D_k not > 0 or +inf: skip
//                 any t - D_k > depth_tol: occluded += 1, skip
//                 with normals n:  e = -d;  cosv = ((n0 e0 + n1 e1) + n2 e2) / sqrt((e0 e0 + e1 e1) + e2 e2);  not cosv > cos_min:
//                 grazing += 1, skip;  w = 1.0, `power` times w = w cosv;   without normals w = 1
//                 fu = u - u0, fv = v - v0;  per channel a = c00 + fu (c10 - c00), b = c01 + fu (c11 - c01), col = a + fv (b - a);
//                 any of the 4 C texels not finite: skip
//                 csum += w col, wsum += w, seen += 1;  w > wbest: wbest = w, cbest = (float)col
//   resolve     MEAN: wsum > 0: (float)(csum / wsum);  BEST: seen > 0: cbest;  else fill, valid = 0;  the four classes to partial[block][4]
//   fill        an invalid vertex with k >= 1 valid neighbours: (float)(s / k), s the fp64 sum of their INPUT colours in list order
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kBakeMaxIndex = (1ll << 31) - 1;     // vertices of a mesh, pixels of a frame: one thread / one int32 offset each
constexpr int kBakeMaxChannels = 16;
constexpr int kBakeMaxPower = 8;

// CT > 0 (1, 3, 4): the channel count at compile time, the colour state (csum, cbest) in registers across the views of the call.
// CT == 0: C <= 16 at run time; 16 channels of state do not fit the registers without scratch, so the colour state is updated in memory view
// by view (the same thread, the same order: the same bytes), in two passes over the channels: are all 4 C texels finite, then the update
template <int CT>
__global__ __launch_bounds__(256) void k_bake_integrate(int V, const float* __restrict__ verts, const float* __restrict__ normals,
                                                        const float* __restrict__ images, const float* __restrict__ depth, int n_views, int H,
                                                        int W, int C, const float* __restrict__ cams, int per_view_cam, double depth_tol,
                                                        double cos_min, int power, double* __restrict__ csum, double* __restrict__ wsum,
                                                        double* __restrict__ wbest, float* __restrict__ cbest, int* __restrict__ seen,
                                                        int* __restrict__ occluded, int* __restrict__ grazing) {
    constexpr int NC = CT ? CT : 1;
    const int nc = CT ? CT : C;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= V) return;
    const double x0 = (double)verts[idx * 3 + 0], x1 = (double)verts[idx * 3 + 1], x2 = (double)verts[idx * 3 + 2];
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (normals) n0 = (double)normals[idx * 3 + 0], n1 = (double)normals[idx * 3 + 1], n2 = (double)normals[idx * 3 + 2];
    double cs[NC], col[NC];
    float cb[NC];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        cs[ch] = 0.0, cb[ch] = 0.0f, col[ch] = 0.0;
        if (CT) cs[ch] = csum[idx * nc + ch], cb[ch] = cbest[idx * nc + ch];
    }
    double ws = wsum[idx], wb = wbest[idx];
    int ns = seen[idx], no = occluded[idx], ng = grazing[idx];
    const long long frame = (long long)H * W;
    const double ulim = (double)(W - 1), vlim = (double)(H - 1);
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
        const double u0 = floor(u), v0 = floor(v);
        if (!(u0 >= 0.0 && u0 + 1.0 <= ulim && v0 >= 0.0 && v0 + 1.0 <= vlim)) continue;
        const int o00 = (int)v0 * W + (int)u0;              // 0 <= u0 <= W - 2, 0 <= v0 <= H - 2: the four offsets lie inside the frame
        const int o10 = o00 + 1, o01 = o00 + W, o11 = o01 + 1;
        const float* __restrict__ dv = depth + (long long)view * frame;
        const float D00 = dv[o00], D10 = dv[o10], D01 = dv[o01], D11 = dv[o11];
        if (!(D00 > 0.0f && D10 > 0.0f && D01 > 0.0f && D11 > 0.0f)) continue;              // NaN, -inf, 0, negative: unknown
        if (D00 == INFINITY || D10 == INFINITY || D01 == INFINITY || D11 == INFINITY) continue;     // background: the silhouette erodes
        if (t - (double)D00 > depth_tol || t - (double)D10 > depth_tol || t - (double)D01 > depth_tol || t - (double)D11 > depth_tol) {
            ++no;
            continue;
        }
        double w = 1.0;
        if (normals) {
            const double e0 = -d0, e1 = -d1, e2 = -d2;
            const double cosv = ((n0 * e0 + n1 * e1) + n2 * e2) / sqrt((e0 * e0 + e1 * e1) + e2 * e2);
            if (!(cosv > cos_min)) {
                ++ng;
                continue;
            }
            for (int k = 0; k < power; ++k) w = w * cosv;
        }
        const double fu = u - u0, fv = v - v0;
        const float* __restrict__ im = images + (long long)view * frame * nc;
        bool finite = true;
        if (CT) {
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                const float c00 = im[(long long)o00 * nc + ch], c10 = im[(long long)o10 * nc + ch], c01 = im[(long long)o01 * nc + ch],
                            c11 = im[(long long)o11 * nc + ch];
                finite = finite && isfinite(c00) && isfinite(c10) && isfinite(c01) && isfinite(c11);
                const double a = (double)c00 + fu * ((double)c10 - (double)c00);
                const double b = (double)c01 + fu * ((double)c11 - (double)c01);
                col[ch] = a + fv * (b - a);
            }
        } else {
            for (int ch = 0; ch < nc; ++ch)
                finite = finite && isfinite(im[(long long)o00 * nc + ch]) && isfinite(im[(long long)o10 * nc + ch]) &&
                         isfinite(im[(long long)o01 * nc + ch]) && isfinite(im[(long long)o11 * nc + ch]);
        }
        if (!finite) continue;
        const bool best = w > wb;                           // strict: the earlier view keeps a tie
        if (CT) {
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                cs[ch] = cs[ch] + w * col[ch];
                if (best) cb[ch] = (float)col[ch];
            }
        } else {
            for (int ch = 0; ch < nc; ++ch) {
                const double c00 = (double)im[(long long)o00 * nc + ch], c10 = (double)im[(long long)o10 * nc + ch],
                             c01 = (double)im[(long long)o01 * nc + ch], c11 = (double)im[(long long)o11 * nc + ch];
                const double a = c00 + fu * (c10 - c00);
                const double b = c01 + fu * (c11 - c01);
                const double one = a + fv * (b - a);
                csum[idx * nc + ch] = csum[idx * nc + ch] + w * one;
                if (best) cbest[idx * nc + ch] = (float)one;
            }
        }
        if (best) wb = w;
        ws = ws + w;
        ++ns;
    }
    if (CT) {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) csum[idx * nc + ch] = cs[ch], cbest[idx * nc + ch] = cb[ch];
    }
    wsum[idx] = ws, wbest[idx] = wb, seen[idx] = ns, occluded[idx] = no, grazing[idx] = ng;
}

// colours + the four classes of this block's vertices (coloured, occluded, grazing, unseen) to partial[block][4]
__global__ __launch_bounds__(256) void k_bake_resolve(int V, int C, const double* __restrict__ csum, const double* __restrict__ wsum,
                                                      const float* __restrict__ cbest, const int* __restrict__ seen,
                                                      const int* __restrict__ occluded, const int* __restrict__ grazing, int blend, float fill,
                                                      float* __restrict__ colors, uint8_t* __restrict__ valid, int* __restrict__ partial) {
    __shared__ int s_counts[4][4];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    int mine[4] = {0, 0, 0, 0};
    if (idx < V) {
        const double ws = wsum[idx];
        const bool ok = blend == MOFA_BAKE_BEST ? seen[idx] > 0 : ws > 0.0;
        for (int ch = 0; ch < C; ++ch) {
            float out = fill;
            if (ok) out = blend == MOFA_BAKE_BEST ? cbest[idx * C + ch] : (float)(csum[idx * C + ch] / ws);
            colors[idx * C + ch] = out;
        }
        valid[idx] = ok ? 1 : 0;
        const bool occ = occluded[idx] > 0, graze = grazing[idx] > 0;
        mine[MOFA_BAKE_COLORED] = ok, mine[MOFA_BAKE_OCCLUDED] = !ok && occ, mine[MOFA_BAKE_GRAZING] = !ok && !occ && graze;
        mine[MOFA_BAKE_UNSEEN] = !ok && !occ && !graze;
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
__global__ __launch_bounds__(256) void k_bake_counts(const int* __restrict__ partial, long long blocks, int64_t* __restrict__ counts) {
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

// one Jacobi step of hole filling: reads `in` / `vin` only, writes `out` / `vout` only.  A list that leaves [0, E) or a neighbour outside
// [0, V) is not dereferenced (the vertex is copied, the neighbour passed over): mesh.py builds the lists from validated faces
__global__ __launch_bounds__(256) void k_bake_fill(int V, int C, const float* __restrict__ in, const uint8_t* __restrict__ vin,
                                                   const int64_t* __restrict__ offsets, const int* __restrict__ nbr, long long E,
                                                   float* __restrict__ out, uint8_t* __restrict__ vout) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    long long k0 = 0, k1 = 0;
    int k = 0;
    if (!vin[i]) {
        k0 = offsets[i], k1 = offsets[i + 1];
        if (k0 < 0 || k1 < k0 || k1 > E) k1 = k0 = 0;
        for (long long q = k0; q < k1; ++q) {
            const int j = nbr[q];
            if (j >= 0 && j < V && vin[j]) ++k;
        }
    }
    if (k == 0) {
        for (int ch = 0; ch < C; ++ch) out[i * C + ch] = in[i * C + ch];
        vout[i] = vin[i];
        return;
    }
    for (int ch = 0; ch < C; ++ch) {
        double s = 0.0;
        for (long long q = k0; q < k1; ++q) {
            const int j = nbr[q];
            if (j >= 0 && j < V && vin[j]) s = s + (double)in[(long long)j * C + ch];
        }
        out[i * C + ch] = (float)(s / (double)k);
    }
    vout[i] = 1;
}

inline long long blocks_of(long long n) { return (n + 255) / 256; }

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_BAKE_SHAPE(what)                                                                                                              \
    MOFA_REQUIRE(V >= 1 && V <= kBakeMaxIndex, what ": V = %lld (want 1 .. 2^31 - 1)", (long long)V);                                         \
    MOFA_REQUIRE(C >= 1 && C <= kBakeMaxChannels, what ": C = %d channels (want 1 .. %d)", (int)C, kBakeMaxChannels)

extern "C" {

int mofa_bake_integrate(const float* verts, const float* normals, int64_t V, const float* images, const float* depth, int64_t n_views, int32_t H,
                        int32_t W, int32_t C, const float* cams, int64_t n_cams, double depth_tol, double cos_min, int32_t power, double* csum,
                        double* wsum, double* wbest, float* cbest, int32_t* seen, int32_t* occluded, int32_t* grazing, void* stream) {
    MOFA_REQUIRE(verts && images && depth && cams && csum && wsum && wbest && cbest && seen && occluded && grazing, "bake_integrate: null pointer");
    MOFA_BAKE_SHAPE("bake_integrate");
    MOFA_REQUIRE(H >= 2 && W >= 2 && (long long)H * W <= kBakeMaxIndex, "bake_integrate: H = %d, W = %d (want H, W >= 2 and H W < 2^31)", (int)H,
                 (int)W);
    MOFA_REQUIRE(n_views >= 1 && n_views <= kBakeMaxIndex, "bake_integrate: n_views = %lld (want 1 .. 2^31 - 1)", (long long)n_views);
    MOFA_REQUIRE(n_cams == 1 || n_cams == n_views, "bake_integrate: %lld cameras for %lld views (want 1 or one per view)", (long long)n_cams,
                 (long long)n_views);
    MOFA_REQUIRE(isfinite(depth_tol) && depth_tol >= 0.0, "bake_integrate: depth_tol = %g (want finite and >= 0)", depth_tol);
    MOFA_REQUIRE(cos_min >= 0.0 && cos_min < 1.0, "bake_integrate: cos_min = %g (want 0 <= cos_min < 1)", cos_min);
    MOFA_REQUIRE(power >= 0 && power <= kBakeMaxPower, "bake_integrate: power = %d (want 0 .. %d)", (int)power, kBakeMaxPower);
    const dim3 grid((unsigned)blocks_of(V)), block(256);
#define MOFA_BAKE_LAUNCH(CT)                                                                                                                  \
    hipLaunchKernelGGL(k_bake_integrate<CT>, grid, block, 0, (hipStream_t)stream, (int)V, verts, normals, images, depth, (int)n_views, (int)H, \
                       (int)W, (int)C, cams, (int)(n_cams != 1), depth_tol, cos_min, (int)power, csum, wsum, wbest, cbest, seen, occluded, grazing)
    switch (C) {
        case 1: MOFA_BAKE_LAUNCH(1); break;
        case 3: MOFA_BAKE_LAUNCH(3); break;
        case 4: MOFA_BAKE_LAUNCH(4); break;
        default: MOFA_BAKE_LAUNCH(0); break;
    }
#undef MOFA_BAKE_LAUNCH
    return check_launch("k_bake_integrate");
}

int mofa_bake_resolve(int64_t V, int32_t C, const double* csum, const double* wsum, const float* cbest, const int32_t* seen,
                      const int32_t* occluded, const int32_t* grazing, int32_t blend, float fill, float* colors, uint8_t* valid, void* workspace,
                      int64_t* counts, void* stream) {
    MOFA_REQUIRE(csum && wsum && cbest && seen && occluded && grazing && colors && valid && workspace && counts, "bake_resolve: null pointer");
    MOFA_BAKE_SHAPE("bake_resolve");
    MOFA_REQUIRE(blend == MOFA_BAKE_MEAN || blend == MOFA_BAKE_BEST, "bake_resolve: blend = %d (want MOFA_BAKE_MEAN or MOFA_BAKE_BEST)", (int)blend);
    const long long blocks = blocks_of(V);
    hipLaunchKernelGGL(k_bake_resolve, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (int)V, (int)C, csum, wsum, cbest, seen, occluded,
                       grazing, (int)blend, fill, colors, valid, (int*)workspace);
    if (int rc = check_launch("k_bake_resolve")) return rc;
    hipLaunchKernelGGL(k_bake_counts, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)workspace, blocks, counts);
    return check_launch("k_bake_counts");
}

int mofa_bake_fill(const float* colors_in, const uint8_t* valid_in, int64_t V, int32_t C, const int64_t* offsets, const int32_t* nbr, int64_t E,
                   float* colors_out, uint8_t* valid_out, void* stream) {
    MOFA_REQUIRE(colors_in && valid_in && offsets && colors_out && valid_out && (nbr || E == 0), "bake_fill: null pointer");
    MOFA_BAKE_SHAPE("bake_fill");
    MOFA_REQUIRE(E >= 0 && E <= kBakeMaxIndex, "bake_fill: E = %lld adjacency entries (want 0 .. 2^31 - 1)", (long long)E);
    MOFA_REQUIRE(colors_in != colors_out && valid_in != valid_out, "bake_fill: the step is double-buffered (input and output must differ)");
    hipLaunchKernelGGL(k_bake_fill, dim3((unsigned)blocks_of(V)), dim3(256), 0, (hipStream_t)stream, (int)V, (int)C, colors_in, valid_in, offsets, nbr,
                       (long long)E, colors_out, valid_out);
    return check_launch("k_bake_fill");
}

}  // extern "C"
