// Ray-side kernels of the MoFaNeRF hot path for gfx950: ray generation, per-ray alpha compositing
// (wavefront prefix product) and importance resampling + merge.  All HBM-bound; one 64-lane wavefront
// owns one ray so the sample buffer is read with fully coalesced 16-byte loads.
// Built with -ffp-contract=off: the reference evaluates these formulas as separate aten ops, so no
// multiply-add may be fused here (SURVEY.md §7 hard part 2).
#include "mofa_composite.h"

extern "C" {   // mofa_mlp.hip: bracket a launch with HIP events when a measurement session is open (bench.py's HBM-side roofline)
int mofa_internal_prof_open(void* stream, int kind);
void mofa_internal_prof_close(void* stream, int kind, double work);
}

namespace mofa {
namespace {


// ---- get_rays (tools/run_nerf_helpers.py:153-168) + viewdirs (render_class.py:399-401) -------------
// `pix_list` (may be NULL): flat pixel indices j * W + i of the n rays (fitting / training batches gather 1-4 k of the H*W
// pixels, run_fit.py:281-293, run_train.py:306-330); NULL = the contiguous range [pix0, pix0 + n).
__global__ __launch_bounds__(256) void k_get_rays(int H, int W, float fx, float fy, float cx, float cy,
                                                  const float* __restrict__ c2w, long long pix0, long long n,
                                                  const int* __restrict__ pix_list, float* __restrict__ rays_o,
                                                  float* __restrict__ rays_d, float* __restrict__ viewdirs) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long long pix = pix_list ? (long long)pix_list[t] : pix0 + t;
    const int j = (int)(pix / W), i = (int)(pix - (long long)j * W);
    float ro[3], rd[3];
    pinhole_ray(i, j, fx, fy, cx, cy, c2w, ro, rd);
    // sqrtf, not __fsqrt_rn: the latter is the hardware's approximate square root here (view directions up to 2 ulp off), sqrtf the correctly
    // rounded one a host restates (k_point_normals)
    const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(rd[0], rd[0]), __fmul_rn(rd[1], rd[1])), __fmul_rn(rd[2], rd[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        rays_o[t * 3 + a] = ro[a];
        rays_d[t * 3 + a] = rd[a];
        if (viewdirs) viewdirs[t * 3 + a] = __fdiv_rn(rd[a], nrm);
    }
}

// d(loss)/d(c2w[3,4]) from the per-ray gradients (the reverse of pinhole_ray):
//   d c2w[a][b] = sum_rays d_rays_d[ray][a] * dirs[ray][b]  (b < 3),   d c2w[a][3] = sum_rays d_rays_o[ray][a].
// One block: thread-local double sums, wavefront butterflies, 4 waves combined through LDS — deterministic, no atomics.
__global__ __launch_bounds__(256) void k_rays_pose_backward(int W, float fx, float fy, float cx, float cy, long long pix0,
                                                            long long n, const int* __restrict__ pix_list,
                                                            const float* __restrict__ d_rays_o,
                                                            const float* __restrict__ d_rays_d, float* __restrict__ d_c2w) {
    __shared__ double part[kWavesPerBlock][12];
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (long long t = threadIdx.x; t < n; t += 256) {
        const long long pix = pix_list ? (long long)pix_list[t] : pix0 + t;
        const int j = (int)(pix / W), i = (int)(pix - (long long)j * W);
        const float dirs[3] = {__fdiv_rn((float)i - cx, fx), -__fdiv_rn((float)j - cy, fy), -1.0f};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double gd = (double)d_rays_d[t * 3 + a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[a * 4 + b] += gd * (double)dirs[b];
            acc[a * 4 + 3] += (double)d_rays_o[t * 3 + a];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double v = wave_sum_d(acc[k]);
        if (lane == 0) part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12) d_c2w[threadIdx.x] = (float)(((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x]);
}

// ---- raw2outputs (models/render_class.py:440-482) --------------------------------------------------
// One wavefront per ray; lane l owns samples [l*SPL, l*SPL+SPL).  The pass itself is mofa_composite.h's.
template <int SPL>
__global__ __launch_bounds__(256) void k_composite(const float* __restrict__ raw, const float* __restrict__ z,
                                                   long long z_row_stride, const float* __restrict__ rays_d,
                                                   const float* __restrict__ noise, long long n_rays, int S,
                                                   int white_bkgd, float* __restrict__ rgb_out,
                                                   float* __restrict__ disp_out, float* __restrict__ acc_out,
                                                   float* __restrict__ depth_out, float* __restrict__ weights_out) {
    CompRay r;
    if (!comp_ray<true>(r, raw, z, z_row_stride, rays_d, noise, n_rays, S)) return;
    CompSlice<SPL> p;
    CompSums sum;
    float carry = 1.0f;   // one pass: comp_lane_T<false> does not touch it
    const float run = comp_load<SPL, true>(r, 0, p);
    comp_accumulate<SPL, true>(r, p, comp_lane_T<false>(run, r.lane, carry), weights_out, sum);
    comp_finish<true>(r, sum, white_bkgd, rgb_out, disp_out, acc_out, depth_out);
}

// Rays with more than 256 samples (the reference has no limit: N_samples / N_importance are free flags, tools/config_parser.py):
// the same wavefront-per-ray scheme walked in PASSES of 256 samples (lane l owns samples [256 p + 4 l, +4) of pass p).  The
// transmittance reaching a pass is carried in a register (product of every earlier (1 - alpha + 1e-10)), the five ray sums are
// accumulated per lane across the passes and reduced once at the end.
__global__ __launch_bounds__(256) void k_composite_long(const float* __restrict__ raw, const float* __restrict__ z,
                                                        long long z_row_stride, const float* __restrict__ rays_d,
                                                        const float* __restrict__ noise, long long n_rays, int S,
                                                        int white_bkgd, float* __restrict__ rgb_out,
                                                        float* __restrict__ disp_out, float* __restrict__ acc_out,
                                                        float* __restrict__ depth_out, float* __restrict__ weights_out) {
    constexpr int SPL = 4;
    CompRay r;
    if (!comp_ray<true>(r, raw, z, z_row_stride, rays_d, noise, n_rays, S)) return;
    CompSums sum;
    float carry = 1.0f;                                   // transmittance in front of the current pass
    for (int base = 0; base < S; base += 64 * SPL) {
        CompSlice<SPL> p;
        const float run = comp_load<SPL, true>(r, base, p);
        comp_accumulate<SPL, true>(r, p, comp_lane_T<true>(run, r.lane, carry), weights_out, sum);
    }
    comp_finish<true>(r, sum, white_bkgd, rgb_out, disp_out, acc_out, depth_out);
}

// ---- raw2outputs without colour: depth / acc / disp / weights from the density alone ------------------------------------------
// The geometry-only render's compositing (mofa_composite_sigma).  `sigma [n_rays,S]` is raw[..., 3] (pre-ReLU) on its own.  These are
// k_composite / k_composite_long instantiated without colour: the same pass, so every output is the bits mofa_composite_forward gives
// for a raw whose channel 3 is sigma (no multiply-add is fused in this translation unit).
template <int SPL>
__global__ __launch_bounds__(256) void k_composite_sigma(const float* __restrict__ sigma, const float* __restrict__ z,
                                                         long long z_row_stride, const float* __restrict__ rays_d,
                                                         const float* __restrict__ noise, long long n_rays, int S,
                                                         float* __restrict__ disp_out, float* __restrict__ acc_out,
                                                         float* __restrict__ depth_out, float* __restrict__ weights_out) {
    CompRay r;
    if (!comp_ray<false>(r, sigma, z, z_row_stride, rays_d, noise, n_rays, S)) return;
    CompSlice<SPL> p;
    CompSums sum;
    float carry = 1.0f;   // one pass: comp_lane_T<false> does not touch it
    const float run = comp_load<SPL, false>(r, 0, p);
    comp_accumulate<SPL, false>(r, p, comp_lane_T<false>(run, r.lane, carry), weights_out, sum);
    comp_finish<false>(r, sum, 0, nullptr, disp_out, acc_out, depth_out);
}

// more than 256 samples: k_composite_long's passes of 256 samples (lane l owns samples [256 p + 4 l, +4) of pass p)
__global__ __launch_bounds__(256) void k_composite_sigma_long(const float* __restrict__ sigma, const float* __restrict__ z,
                                                              long long z_row_stride, const float* __restrict__ rays_d,
                                                              const float* __restrict__ noise, long long n_rays, int S,
                                                              float* __restrict__ disp_out, float* __restrict__ acc_out,
                                                              float* __restrict__ depth_out, float* __restrict__ weights_out) {
    constexpr int SPL = 4;
    CompRay r;
    if (!comp_ray<false>(r, sigma, z, z_row_stride, rays_d, noise, n_rays, S)) return;
    CompSums sum;
    float carry = 1.0f;                                   // transmittance in front of the current pass
    for (int base = 0; base < S; base += 64 * SPL) {
        CompSlice<SPL> p;
        const float run = comp_load<SPL, false>(r, base, p);
        comp_accumulate<SPL, false>(r, p, comp_lane_T<true>(run, r.lane, carry), weights_out, sum);
    }
    comp_finish<false>(r, sum, 0, nullptr, disp_out, acc_out, depth_out);
}

// ---- the points of a pass: p = o + d * z, multiply and add rounded separately (the point the network's layer-0 prologue forms) ----
__global__ __launch_bounds__(256) void k_ray_points(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                    const float* __restrict__ z, long long z_row_stride, long long n_samples, int S,
                                                    float* __restrict__ pts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples) return;
    const long long r = e / S;
    const int s = (int)(e - r * S);
    const float zv = z[r * z_row_stride + s];
#pragma unroll
    for (int a = 0; a < 3; ++a) pts[e * 3 + a] = __fadd_rn(rays_o[r * 3 + a], __fmul_rn(rays_d[r * 3 + a], zv));
}

// ---- median termination depth: the first sample at which the accumulated weight reaches a threshold ---------------------------------
// One wavefront per ray, k_composite_sigma's lane-to-sample assignment (lane l owns samples [l*SPL, l*SPL+SPL)).  The inclusive prefix
// sum C_i = w_0 + ... + w_i is formed as (sum of the lanes in front, a 6-step wavefront scan of the lanes' totals) + (the lane's own
// running sum): every C_i is an fp32 sum of exactly w_0..w_i (slots past S add an exact 0), so |C_i - exact| <= (S-1) 2^-24 sum|w|.
// index = the least i with C_i >= threshold (a wavefront minimum over each lane's first hit), -1 if there is none; a NaN weight makes
// every later C_i NaN, which compares false.  depth_med = z[index], z[S-1] for -1.
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

constexpr int kNoIndex = 0x7fffffff;

// the least sample index of this pass whose prefix sum reaches the threshold (kNoIndex: none), the same value in every lane;
// `carry` = the sum of the passes in front on entry, of the passes up to and including this one on return
template <int SPL>
__device__ __forceinline__ int median_pass(const float* __restrict__ wr, int base, int S, float threshold, int lane, float& carry) {
    float run[SPL];
    const int s0 = base + lane * SPL;
    float tot = 0.f;
#pragma unroll
    for (int t = 0; t < SPL; ++t) {
        const float w = (s0 + t < S) ? wr[s0 + t] : 0.f;
        tot = t == 0 ? w : tot + w;
        run[t] = tot;
    }
    float incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if (lane >= o) incl = incl + up;
    }
    float front = __shfl_up(incl, 1, 64);
    front = lane == 0 ? carry : carry + front;
    carry = carry + __shfl(incl, 63, 64);
    int hit = kNoIndex;
#pragma unroll
    for (int t = SPL - 1; t >= 0; --t)
        if (s0 + t < S && front + run[t] >= threshold) hit = s0 + t;
    return wave_min_i(hit);
}

template <int SPL>
__global__ __launch_bounds__(256) void k_depth_median(const float* __restrict__ weights, const float* __restrict__ z,
                                                      long long z_row_stride, long long n_rays, int S, float threshold,
                                                      float* __restrict__ depth_med, int* __restrict__ index) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    float carry = 0.f;
    const int hit = median_pass<SPL>(weights + ray * (long long)S, 0, S, threshold, lane, carry);
    if (lane == 0) {
        const float* zr = z + ray * z_row_stride;
        index[ray] = hit == kNoIndex ? -1 : hit;
        depth_med[ray] = zr[hit == kNoIndex ? S - 1 : hit];
    }
}

// more than 256 samples: passes of 256 samples (lane l owns samples [256 p + 4 l, +4) of pass p), the sum of the passes in front carried
__global__ __launch_bounds__(256) void k_depth_median_long(const float* __restrict__ weights, const float* __restrict__ z,
                                                           long long z_row_stride, long long n_rays, int S, float threshold,
                                                           float* __restrict__ depth_med, int* __restrict__ index) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    float carry = 0.f;
    int hit = kNoIndex;
    for (int base = 0; base < S && hit == kNoIndex; base += 256)      // (hit is the same in every lane: the wavefront leaves together)
        hit = median_pass<4>(weights + ray * (long long)S, base, S, threshold, lane, carry);
    if (lane == 0) {
        const float* zr = z + ray * z_row_stride;
        index[ray] = hit == kNoIndex ? -1 : hit;
        depth_med[ray] = zr[hit == kNoIndex ? S - 1 : hit];
    }
}

// ---- screen-space normals of a point map ---------------------------------------------------------------------------------------------
// One thread per pixel of an H x W map.  A pixel is usable iff acc >= acc_min (NaN is not).  Along each image axis the difference is
// central (P[+1] - P[-1]) when both neighbours exist and are usable, else forward (P[+1] - P), else backward (P - P[-1]), else the pixel
// is invalid.  n = du x dv (two rounded products and one rounded subtraction per component), divided by its rounded length, turned to
// face the camera (n . d <= 0); the square root and the divisions are the correctly rounded ones.  Every output element is written: invalid pixels get (0,0,0) and valid = 0.
__device__ __forceinline__ bool axis_difference(const float* __restrict__ P, const float* __restrict__ acc, float acc_min, long long p,
                                                long long step, bool has_prev, bool has_next, float out[3]) {
    const bool prev = has_prev && acc[p - step] >= acc_min, next = has_next && acc[p + step] >= acc_min;
    if (!prev && !next) return false;
    const long long a = next ? p + step : p, b = prev && next ? p - step : (next ? p : p - step);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = __fsub_rn(P[a * 3 + k], P[b * 3 + k]);
    return true;
}

__global__ __launch_bounds__(256) void k_point_normals(const float* __restrict__ points, const float* __restrict__ acc,
                                                       const float* __restrict__ rays_d, int H, int W, float acc_min,
                                                       float* __restrict__ normals, unsigned char* __restrict__ valid) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int r = (int)(p / W), c = (int)(p - (long long)r * W);
    float du[3], dv[3], n[3] = {0.f, 0.f, 0.f};
    bool ok = acc[p] >= acc_min;
    ok = ok && axis_difference(points, acc, acc_min, p, 1, c > 0, c + 1 < W, du);
    ok = ok && axis_difference(points, acc, acc_min, p, W, r > 0, r + 1 < H, dv);
    if (ok) {
        const float nx = __fsub_rn(__fmul_rn(du[1], dv[2]), __fmul_rn(du[2], dv[1]));
        const float ny = __fsub_rn(__fmul_rn(du[2], dv[0]), __fmul_rn(du[0], dv[2]));
        const float nz = __fsub_rn(__fmul_rn(du[0], dv[1]), __fmul_rn(du[1], dv[0]));
        // sqrtf, not __fsqrt_rn: the latter is the hardware's approximate square root here, sqrtf the correctly rounded one a host restates
        const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
        ok = len > 0.f;
        if (ok) {
            n[0] = __fdiv_rn(nx, len), n[1] = __fdiv_rn(ny, len), n[2] = __fdiv_rn(nz, len);
            const float s = __fadd_rn(__fadd_rn(__fmul_rn(n[0], rays_d[p * 3]), __fmul_rn(n[1], rays_d[p * 3 + 1])),
                                      __fmul_rn(n[2], rays_d[p * 3 + 2]));
            if (s > 0.f) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[p * 3 + k] = n[k];
    valid[p] = ok ? 1 : 0;
}

// ---- sample_pdf + sort(cat) + std (tools/run_nerf_helpers.py:203-247; render_class.py:324-328,345) ----
// One wavefront per ray.  B = S-1 bin edges z_mid, B-1 = S-2 interior weights.
// cdf follows the CPU reference: cumsum accumulates in double and rounds every prefix to float.
// LDS per ray (= per wavefront): S + Ni merged positions, S bin edges, S cdf entries.  The block carries as many waves (1, 2
// or 4) as fit in 64 KiB, so the shipped 64 + 64 runs four rays per workgroup and a 4096 + 4096 ray still has a wave to itself.
constexpr int kPdfLdsFloats = 16384;   // 64 KiB

// BINS = true is the plain `sample_pdf(bins, weights, N)` entry (mofa_sample_pdf): `z` holds the B bin edges themselves
// (S := B), `weights` the B-1 bin weights, and nothing is merged (z_fine / z_std may be NULL).
inline long long pdf_lds_floats(int S, int Ni) { return 3ll * S + Ni; }
inline int pdf_waves(int S, int Ni) {
    const long long per = pdf_lds_floats(S, Ni);
    return per * 4 <= kPdfLdsFloats ? 4 : (per * 2 <= kPdfLdsFloats ? 2 : 1);
}

template <bool BINS>
__global__ __launch_bounds__(256) void k_sample_pdf_merge(const float* __restrict__ z, long long z_row_stride,
                                                          const float* __restrict__ weights,
                                                          const float* __restrict__ u, long long u_row_stride,
                                                          long long n_rays, int S, int Ni,
                                                          float* __restrict__ z_samples, float* __restrict__ z_fine,
                                                          float* __restrict__ z_std) {
    extern __shared__ __attribute__((aligned(16))) float s_pdf[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * (blockDim.x >> 6) + wv;
    if (ray >= n_rays) return;  // wave-uniform; no block-level barrier is used below
    float* all = s_pdf + (long long)wv * (3ll * S + Ni);  // [0,S): coarse z, [S,S+Ni): new samples
    float* bins = all + S + Ni;                            // [S]
    float* cdf = bins + S;                                 // [S]
    const float* zr = z + ray * z_row_stride;
    const int B = BINS ? S : S - 1;   // len(bins) == len(cdf)
    const int NW = B - 1;             // bin weights (the interior weights [1:-1] of the S coarse samples)
    const float* wr = BINS ? weights + ray * (long long)NW - 1 : weights + ray * (long long)S;   // wr[i + 1] = weight of bin i

    for (int s = lane; s < S; s += 64) all[s] = zr[s];
    __builtin_amdgcn_wave_barrier();
    for (int b = lane; b < B; b += 64) bins[b] = BINS ? all[b] : 0.5f * (all[b + 1] + all[b]);

    // pdf = (w + 1e-5) / sum(w + 1e-5); cdf = [0, cumsum(pdf)]
    double part = 0.0;
    for (int i = lane; i < NW; i += 64) part += (double)(wr[i + 1] + 1e-5f);
    const float wsum = (float)wave_sum_d(part);
    double carry = 0.0;
    if (lane == 0) cdf[0] = 0.f;
    for (int base = 0; base < NW; base += 64) {
        const int i = base + lane;
        double v = (i < NW) ? (double)__fdiv_rn(wr[i + 1] + 1e-5f, wsum) : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double up = __shfl_up(v, o, 64);
            if (lane >= o) v += up;
        }
        v += carry;
        if (i < NW) cdf[i + 1] = (float)v;
        carry = __shfl(v, 63, 64);
    }
    __builtin_amdgcn_wave_barrier();

    // invert the cdf at each u
    double m1 = 0.0;
    for (int j = lane; j < Ni; j += 64) {
        const float uu = u[ray * u_row_stride + j];
        int lo = 0, hi = B;  // first index with cdf[idx] > uu  (searchsorted right=True)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] > uu) hi = mid; else lo = mid + 1;
        }
        const int below = max(lo - 1, 0), above = min(lo, B - 1);
        const float c0 = cdf[below], c1 = cdf[above], b0 = bins[below], b1 = bins[above];
        float denom = c1 - c0;
        if (denom < 1e-5f) denom = 1.0f;
        const float t = __fdiv_rn(uu - c0, denom);
        const float smp = b0 + t * (b1 - b0);
        all[S + j] = smp;
        z_samples[ray * (long long)Ni + j] = smp;
        m1 += (double)smp;
    }
    // population std of the new samples (torch.std(unbiased=False))
    const double mean = wave_sum_d(m1) / (double)Ni;
    __builtin_amdgcn_wave_barrier();
    double m2 = 0.0;
    for (int j = lane; j < Ni; j += 64) {
        const double dlt = (double)all[S + j] - mean;
        m2 += dlt * dlt;
    }
    m2 = wave_sum_d(m2);
    if (lane == 0 && z_std) z_std[ray] = (float)sqrt(m2 / (double)Ni);
    if (BINS || !z_fine) return;

    // merge by rank: position = #(smaller) + #(equal with a lower index), a NaN after every number and behind the NaNs of a lower index —
    // torch.sort's result for ANY input (the stochastic mode's samples arrive unsorted; NaN compares false both ways, so without its own
    // rule every NaN would claim slot 0 and leave the row's last slots unwritten).  When both runs are already non-decreasing (always the
    // coarse positions; the new samples whenever u is — the det mode's linspace — up to an ulp at a bin edge, which is why it is CHECKED,
    // not assumed) the same rank is
    //   coarse e:  e + #(samples < v)        sample j:  j + #(coarse <= v)
    // i.e. one binary search per element (7 dependent LDS reads) instead of a pass over all N positions (round 6: the O(N^2) pass was
    // two thirds of this kernel's instructions; NaN fails the check and takes the general pass).
    const int N = S + Ni;
    bool runs_sorted = true;
    for (int e = lane; e < N; e += 64) {
        const int last = e < S ? S - 1 : N - 1;
        const float v = all[e];
        // a run's last element has no neighbour to fail against: without v == v a lone NaN sample (Ni = 1) would pass
        runs_sorted = runs_sorted && (e < last ? v <= all[e + 1] : v == v);
    }
    if (__all(runs_sorted ? 1 : 0)) {
        for (int e = lane; e < N; e += 64) {
            const float v = all[e];
            int lo, hi;
            if (e < S) {                      // first sample not below v
                lo = S, hi = N;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (all[mid] < v) lo = mid + 1; else hi = mid;
                }
                z_fine[ray * (long long)N + e + (lo - S)] = v;
            } else {                          // first coarse position above v
                lo = 0, hi = S;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (all[mid] <= v) lo = mid + 1; else hi = mid;
                }
                z_fine[ray * (long long)N + (e - S) + lo] = v;
            }
        }
        return;
    }
    for (int e = lane; e < N; e += 64) {
        const float v = all[e];
        int rank = 0;
        if (v == v) {
            for (int k = 0; k < N; ++k) {
                const float o = all[k];
                rank += (o < v || (o == v && k < e)) ? 1 : 0;
            }
        } else {
            for (int k = 0; k < N; ++k) {
                const float o = all[k];
                rank += (o == o || k < e) ? 1 : 0;
            }
        }
        z_fine[ray * (long long)N + rank] = v;
    }
}

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace mofa

using namespace mofa;

extern "C" {

int mofa_get_rays(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* c2w, int64_t pix0,
                  int64_t n, float* rays_o, float* rays_d, float* viewdirs, void* stream) {
    MOFA_REQUIRE(c2w && rays_o && rays_d, "get_rays: null pointer");
    MOFA_REQUIRE(H > 0 && W > 0 && n > 0 && pix0 >= 0 && pix0 + n <= (int64_t)H * W, "get_rays: pixel range");
    hipLaunchKernelGGL(k_get_rays, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, H, W, fx, fy, cx, cy,
                       c2w, (long long)pix0, (long long)n, (const int*)nullptr, rays_o, rays_d, viewdirs);
    return check_launch("k_get_rays");
}

int mofa_get_rays_at(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* c2w, const int32_t* pixels,
                     int64_t n, float* rays_o, float* rays_d, float* viewdirs, void* stream) {
    MOFA_REQUIRE(c2w && pixels && rays_o && rays_d, "get_rays_at: null pointer");
    MOFA_REQUIRE(H > 0 && W > 0 && n > 0 && (int64_t)H * W < (1ll << 31), "get_rays_at: bad image size / count");
    hipLaunchKernelGGL(k_get_rays, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, H, W, fx, fy, cx, cy,
                       c2w, 0ll, (long long)n, (const int*)pixels, rays_o, rays_d, viewdirs);
    return check_launch("k_get_rays(at)");
}

int mofa_rays_pose_backward(int32_t W, float fx, float fy, float cx, float cy, const int32_t* pixels, int64_t pix0, int64_t n,
                            const float* d_rays_o, const float* d_rays_d, float* d_c2w, void* stream) {
    MOFA_REQUIRE(d_rays_o && d_rays_d && d_c2w && W > 0 && n > 0, "rays_pose_backward: bad arguments");
    hipLaunchKernelGGL(k_rays_pose_backward, dim3(1), dim3(256), 0, (hipStream_t)stream, W, fx, fy, cx, cy, (long long)pix0,
                       (long long)n, (const int*)pixels, d_rays_o, d_rays_d, d_c2w);
    return check_launch("k_rays_pose_backward");
}

int mofa_composite_forward(const float* raw, const float* z, int64_t z_row_stride, const float* rays_d,
                           const float* noise, int64_t n_rays, int32_t S, int32_t white_bkgd, float* rgb,
                           float* disp, float* acc, float* depth, float* weights, void* stream) {
    MOFA_REQUIRE(raw && z && rays_d && rgb && disp && acc && depth && weights, "composite_forward: null pointer");
    MOFA_REQUIRE(n_rays > 0 && S >= 2, "composite_forward: need S >= 2 (got %d)", S);
    const dim3 grid(blocks_for(n_rays, kWavesPerBlock)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int pkind = S <= 64 ? 8 : (S <= 128 ? 9 : -1);            // the two instantiations of the benchmark's passes
    const int prof = pkind >= 0 ? mofa_internal_prof_open(stream, pkind) : 0;
    if (prof < 0) return MOFA_EHIP;
#define MOFA_COMPOSITE(SPL)                                                                                     \
    hipLaunchKernelGGL((k_composite<SPL>), grid, block, 0, st, raw, z, (long long)z_row_stride, rays_d, noise, \
                       (long long)n_rays, S, white_bkgd, rgb, disp, acc, depth, weights)
    if (S <= 64) MOFA_COMPOSITE(1);
    else if (S <= 128) MOFA_COMPOSITE(2);
    else if (S <= 256) MOFA_COMPOSITE(4);
    else
        hipLaunchKernelGGL(k_composite_long, grid, block, 0, st, raw, z, (long long)z_row_stride, rays_d, noise, (long long)n_rays, S,
                           white_bkgd, rgb, disp, acc, depth, weights);
#undef MOFA_COMPOSITE
    if (prof) mofa_internal_prof_close(stream, pkind, (double)n_rays);
    return check_launch("k_composite");
}

int mofa_composite_sigma(const float* sigma, const float* z, int64_t z_row_stride, const float* rays_d, const float* noise,
                         int64_t n_rays, int32_t S, float* disp, float* acc, float* depth, float* weights, void* stream) {
    MOFA_REQUIRE(sigma && z && rays_d && disp && acc && depth && weights, "composite_sigma: null pointer");
    MOFA_REQUIRE(n_rays > 0 && S >= 2, "composite_sigma: need S >= 2 (got %d)", S);
    MOFA_REQUIRE(z_row_stride == 0 || z_row_stride == S, "composite_sigma: z_row_stride = %lld with S = %d (want 0 or S)",
                 (long long)z_row_stride, (int)S);
    MOFA_REQUIRE(n_rays < (1ll << 31) && n_rays * (int64_t)S < (1ll << 31), "composite_sigma: %lld rays x %d samples (want fewer than 2^31 samples)",
                 (long long)n_rays, (int)S);
    const dim3 grid(blocks_for(n_rays, kWavesPerBlock)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define MOFA_COMPOSITE_SIGMA(SPL)                                                                                         \
    hipLaunchKernelGGL((k_composite_sigma<SPL>), grid, block, 0, st, sigma, z, (long long)z_row_stride, rays_d, noise, \
                       (long long)n_rays, S, disp, acc, depth, weights)
    if (S <= 64) MOFA_COMPOSITE_SIGMA(1);
    else if (S <= 128) MOFA_COMPOSITE_SIGMA(2);
    else if (S <= 256) MOFA_COMPOSITE_SIGMA(4);
    else
        hipLaunchKernelGGL(k_composite_sigma_long, grid, block, 0, st, sigma, z, (long long)z_row_stride, rays_d, noise, (long long)n_rays, S,
                           disp, acc, depth, weights);
#undef MOFA_COMPOSITE_SIGMA
    return check_launch("k_composite_sigma");
}

int mofa_ray_points(const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride, int64_t n_rays, int32_t S,
                    float* pts, void* stream) {
    MOFA_REQUIRE(rays_o && rays_d && z && pts, "ray_points: null pointer");
    MOFA_REQUIRE(n_rays >= 1 && S >= 1 && n_rays < (1ll << 31) && n_rays * (int64_t)S < (1ll << 31),
                 "ray_points: %lld rays x %d samples (want at least one and fewer than 2^31 samples)", (long long)n_rays, (int)S);
    MOFA_REQUIRE(z_row_stride == 0 || z_row_stride == S, "ray_points: z_row_stride = %lld with S = %d (want 0 or S)",
                 (long long)z_row_stride, (int)S);
    const long long n = (long long)n_rays * S;
    hipLaunchKernelGGL(k_ray_points, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, z,
                       (long long)z_row_stride, n, (int)S, pts);
    return check_launch("k_ray_points");
}

int mofa_depth_median(const float* weights, const float* z, int64_t z_row_stride, int64_t n_rays, int32_t S, float threshold,
                      float* depth_med, int32_t* index, void* stream) {
    MOFA_REQUIRE(weights && z && depth_med && index, "depth_median: null pointer");
    MOFA_REQUIRE(n_rays >= 1 && S >= 1 && n_rays < (1ll << 31) && n_rays * (int64_t)S < (1ll << 31),
                 "depth_median: %lld rays x %d samples (want at least one and fewer than 2^31 samples)", (long long)n_rays, (int)S);
    MOFA_REQUIRE(z_row_stride == 0 || z_row_stride == S, "depth_median: z_row_stride = %lld with S = %d (want 0 or S)",
                 (long long)z_row_stride, (int)S);
    MOFA_REQUIRE(threshold > 0.f && threshold <= 3.402823466e38f, "depth_median: threshold = %g (want finite and > 0)", (double)threshold);
    const dim3 grid(blocks_for(n_rays, kWavesPerBlock)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define MOFA_DEPTH_MEDIAN(SPL)                                                                                                  \
    hipLaunchKernelGGL((k_depth_median<SPL>), grid, block, 0, st, weights, z, (long long)z_row_stride, (long long)n_rays, (int)S, \
                       threshold, depth_med, (int*)index)
    if (S <= 64) MOFA_DEPTH_MEDIAN(1);
    else if (S <= 128) MOFA_DEPTH_MEDIAN(2);
    else if (S <= 256) MOFA_DEPTH_MEDIAN(4);
    else
        hipLaunchKernelGGL(k_depth_median_long, grid, block, 0, st, weights, z, (long long)z_row_stride, (long long)n_rays, (int)S,
                           threshold, depth_med, (int*)index);
#undef MOFA_DEPTH_MEDIAN
    return check_launch("k_depth_median");
}

int mofa_point_normals(const float* points, const float* acc, const float* rays_d, int32_t H, int32_t W, float acc_min, float* normals,
                       uint8_t* valid, void* stream) {
    MOFA_REQUIRE(points && acc && rays_d && normals && valid, "point_normals: null pointer");
    MOFA_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 31), "point_normals: a %d x %d map (want at least 1 x 1 and fewer than 2^31 pixels)",
                 (int)H, (int)W);
    MOFA_REQUIRE(acc_min >= -3.402823466e38f && acc_min <= 3.402823466e38f, "point_normals: acc_min = %g (want a finite value)", (double)acc_min);
    hipLaunchKernelGGL(k_point_normals, dim3(blocks_for((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, points, acc, rays_d,
                       (int)H, (int)W, acc_min, normals, (unsigned char*)valid);
    return check_launch("k_point_normals");
}

int mofa_sample_pdf_merge(const float* z, int64_t z_row_stride, const float* weights, const float* u,
                          int64_t u_row_stride, int64_t n_rays, int32_t S, int32_t Ni, float* z_samples,
                          float* z_fine, float* z_std, void* stream) {
    MOFA_REQUIRE(z && weights && u && z_samples && z_fine && z_std, "sample_pdf_merge: null pointer");
    MOFA_REQUIRE(n_rays > 0 && S >= 4 && Ni >= 1 && pdf_lds_floats(S, Ni) <= kPdfLdsFloats,
                 "sample_pdf_merge: need S >= 4, Ni >= 1 and 3 S + Ni <= %d (one ray's positions, bins and cdf live in 64 KiB of LDS); got %d, %d",
                 kPdfLdsFloats, S, Ni);
    const int wv = pdf_waves(S, Ni);
    const int prof = mofa_internal_prof_open(stream, 10);
    if (prof < 0) return MOFA_EHIP;
    hipLaunchKernelGGL(k_sample_pdf_merge<false>, dim3(blocks_for(n_rays, wv)), dim3(64 * wv), (size_t)wv * pdf_lds_floats(S, Ni) * sizeof(float),
                       (hipStream_t)stream, z, (long long)z_row_stride, weights, u, (long long)u_row_stride,
                       (long long)n_rays, S, Ni, z_samples, z_fine, z_std);
    if (prof) mofa_internal_prof_close(stream, 10, (double)n_rays);
    return check_launch("k_sample_pdf_merge");
}

int mofa_sample_pdf(const float* bins, int64_t bins_row_stride, const float* weights, const float* u, int64_t u_row_stride,
                    int64_t n_rays, int32_t n_bins, int32_t Ni, float* samples, void* stream) {
    MOFA_REQUIRE(bins && weights && u && samples, "sample_pdf: null pointer");
    MOFA_REQUIRE(n_rays > 0 && n_bins >= 3 && Ni >= 1 && pdf_lds_floats(n_bins, Ni) <= kPdfLdsFloats,
                 "sample_pdf: need n_bins >= 3, Ni >= 1 and 3 n_bins + Ni <= %d; got %d, %d", kPdfLdsFloats, n_bins, Ni);
    const int wv = pdf_waves(n_bins, Ni);
    hipLaunchKernelGGL(k_sample_pdf_merge<true>, dim3(blocks_for(n_rays, wv)), dim3(64 * wv), (size_t)wv * pdf_lds_floats(n_bins, Ni) * sizeof(float),
                       (hipStream_t)stream, bins, (long long)bins_row_stride, weights, u, (long long)u_row_stride,
                       (long long)n_rays, n_bins, Ni, samples, (float*)nullptr, (float*)nullptr);
    return check_launch("k_sample_pdf");
}

}  // extern "C"
