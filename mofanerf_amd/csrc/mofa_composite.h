// raw2outputs (models/render_class.py:440-482) as the pieces every compositing kernel is made of: k_composite<SPL> / k_composite_long,
// their colourless twins k_composite_sigma<SPL> / k_composite_sigma_long (mofa_rays.hip) and k_composite_backward<SPL> /
// k_composite_backward_long (mofa_bwd.hip), whose first half recomputes the forward.
// One wavefront per ray, walked in passes of 64 * SPL samples: lane l owns samples [base + l*SPL, +SPL) of the pass at `base` (the short
// forms are one pass at 0).  T_i = prod_{j<i} (1 - alpha_j + 1e-10) is an in-lane running product combined with a 6-step wavefront
// exclusive prefix product and, across passes, a carry register.
// COLOUR = false takes sigma from a row of its own and leaves the colour lines out AT COMPILE TIME; nothing here branches at run time on
// the kernel it serves.  Both including files are built with -ffp-contract=off, so the same source line is the same rounded operations
// everywhere: that is what makes the sigma twin and the backward's recomputation bit-identical to k_composite.
#pragma once
#include "mofa_common.h"

namespace mofa {
namespace {

constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the ray of this wavefront
struct CompRay {
    int lane, S;
    long long ray, row;   // row = ray * S: the ray's first sample in the [n_rays, S] arrays
    float dx, dy, dz, dnorm;
    const float* zr;      // the ray's sample positions
    const float* src;     // COLOUR: the ray's raw rows (one f32x4 per sample); else its sigma row (raw[..., 3], pre-ReLU)
    const float* noise;   // [n_rays, S] or NULL
};

// false: no such ray (wave-uniform; the wavefront leaves)
template <bool COLOUR>
__device__ __forceinline__ bool comp_ray(CompRay& r, const float* __restrict__ src, const float* __restrict__ z, long long z_row_stride,
                                         const float* __restrict__ rays_d, const float* __restrict__ noise, long long n_rays, int S) {
    r.lane = threadIdx.x & 63, r.S = S;
    r.ray = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (r.ray >= n_rays) return false;
    r.dx = rays_d[r.ray * 3], r.dy = rays_d[r.ray * 3 + 1], r.dz = rays_d[r.ray * 3 + 2];
    r.dnorm = __fsqrt_rn(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz);
    r.zr = z + r.ray * z_row_stride;
    r.row = r.ray * (long long)S;
    r.src = src + r.row * (COLOUR ? 4 : 1);
    r.noise = noise;
    return true;
}

// a lane's SPL samples of one pass.  sig / dlt are the backward's; c* exist with COLOUR only.  What a kernel does not read the compiler drops.
template <int SPL>
struct CompSlice {
    int s0;                                 // the lane's first sample
    float zv[SPL + 1], alpha[SPL];
    float sig[SPL];                         // sigma (+ noise), pre-ReLU (its sign decides the backward's gate)
    float dlt[SPL];                         // z step to the next sample (1e10 behind the last), not yet scaled by |rays_d|
    float cr[SPL], cg[SPL], cb[SPL];
};

// fills the slice; returns this lane's product of (1 - alpha + 1e-10)
template <int SPL, bool COLOUR>
__device__ __forceinline__ float comp_load(const CompRay& r, int base, CompSlice<SPL>& p) {
    const int S = r.S;
    p.s0 = base + r.lane * SPL;
#pragma unroll
    for (int t = 0; t <= SPL; ++t) p.zv[t] = (p.s0 + t < S) ? r.zr[p.s0 + t] : 0.f;
    float run = 1.0f;
#pragma unroll
    for (int t = 0; t < SPL; ++t) {
        const int s = p.s0 + t;
        if (s < S) {
            f32x4 v;
            float sg;
            if constexpr (COLOUR) v = ((const f32x4*)r.src)[s], sg = v.w;
            else sg = r.src[s];
            p.dlt[t] = (s + 1 < S) ? (p.zv[t + 1] - p.zv[t]) : 1e10f;
            if (r.noise) sg = sg + r.noise[r.row + s];
            p.sig[t] = sg;
            p.alpha[t] = 1.0f - expf(-relu_np(sg) * (p.dlt[t] * r.dnorm));
            if constexpr (COLOUR) {
                p.cr[t] = 1.0f / (1.0f + expf(-v.x));
                p.cg[t] = 1.0f / (1.0f + expf(-v.y));
                p.cb[t] = 1.0f / (1.0f + expf(-v.z));
            }
            run = run * ((1.0f - p.alpha[t]) + 1e-10f);
        } else {
            p.alpha[t] = 0.f, p.sig[t] = 0.f, p.dlt[t] = 0.f;
            if constexpr (COLOUR) p.cr[t] = p.cg[t] = p.cb[t] = 0.f;
        }
    }
    return run;
}

// The transmittance in front of this lane's first sample: the exclusive prefix product of the lanes' `run`.  CARRY (the long forms):
// times `carry`, the transmittance in front of the pass, which leaves multiplied by the pass's total; the short forms do not touch it.
template <bool CARRY>
__device__ __forceinline__ float comp_lane_T(float run, int lane, float& carry) {
    float incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if (lane >= o) incl = incl * up;
    }
    float T = __shfl_up(incl, 1, 64);
    if (lane == 0) T = 1.0f;
    if constexpr (CARRY) {
        T = carry * T;
        carry = carry * __shfl(incl, 63, 64);
    }
    return T;
}

// a lane's partial sums of the ray's outputs (r, g, b with COLOUR only)
struct CompSums {
    float r = 0.f, g = 0.f, b = 0.f, d = 0.f, a = 0.f;
};

// forward: stores the slice's weights and adds its terms to the lane's sums
template <int SPL, bool COLOUR>
__device__ __forceinline__ void comp_accumulate(const CompRay& r, const CompSlice<SPL>& p, float T, float* __restrict__ weights_out,
                                                CompSums& sum) {
#pragma unroll
    for (int t = 0; t < SPL; ++t) {
        const int s = p.s0 + t;
        if (s < r.S) {
            const float w = p.alpha[t] * T;
            weights_out[r.row + s] = w;
            if constexpr (COLOUR) sum.r += w * p.cr[t], sum.g += w * p.cg[t], sum.b += w * p.cb[t];
            sum.d += w * p.zv[t];
            sum.a += w;
            T = T * ((1.0f - p.alpha[t]) + 1e-10f);
        }
    }
}

// forward: reduces the lanes' sums and writes the ray's outputs from lane 0
template <bool COLOUR>
__device__ __forceinline__ void comp_finish(const CompRay& r, CompSums sum, int white_bkgd, float* __restrict__ rgb_out,
                                            float* __restrict__ disp_out, float* __restrict__ acc_out, float* __restrict__ depth_out) {
    if constexpr (COLOUR) sum.r = wave_sum(sum.r), sum.g = wave_sum(sum.g), sum.b = wave_sum(sum.b);
    sum.d = wave_sum(sum.d), sum.a = wave_sum(sum.a);
    if (r.lane != 0) return;
    if constexpr (COLOUR) {
        if (white_bkgd) {
            const float bg = 1.0f - sum.a;
            sum.r += bg, sum.g += bg, sum.b += bg;
        }
        rgb_out[r.ray * 3] = sum.r, rgb_out[r.ray * 3 + 1] = sum.g, rgb_out[r.ray * 3 + 2] = sum.b;
    }
    const float q = __fdiv_rn(sum.d, sum.a);  // 0/0 -> NaN, and torch.max propagates it (render_class.py:476)
    disp_out[r.ray] = (q != q) ? q : __fdiv_rn(1.0f, fmaxf(1e-10f, q));
    acc_out[r.ray] = sum.a;
    depth_out[r.ray] = sum.d;
}

}  // namespace
}  // namespace mofa
