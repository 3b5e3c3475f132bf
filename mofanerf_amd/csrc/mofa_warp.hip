// Non-rigid mesh registration for the geometry export (gfx950): the linear step of stiffness-regularised ICP with a translation per vertex.
// mesh.py drives the loop (mesh.warp, mesh.warp_to): it moves the template (apply), asks closest_points for the correspondences, decides
// the rejections, builds the normal equations (D + alpha L (x) I3) d = b per vertex (system) and solves them by Jacobi-preconditioned
// conjugate gradients (solve): a fixed sequence of cg_iterations steps enqueued without a host read, stopped by a sticky flag in device
// memory.  Nothing here waits on another thread or workgroup and there is no atomic of any kind: every sum has a fixed order that does not
// depend on the launch geometry, so the same input gives the same bytes.  Every kernel checks the indices it dereferences: a vertex with a
// bad list or neighbour writes nothing and is counted per workgroup.  All arithmetic is fp64 (the fp32 inputs widened), every operation
// rounded separately (the build pins -ffp-contract=off).  The order of operations is the header's (include/mofanerf_hip.h); in short:
//
//   apply    y[i][k] = (float)((double)v[i][k] + d[i][k])
//   system   u = c - v, r = y - c (widened);  live = w > 0 and (plane, by face) the face and its vertices lie inside the target
//              point:  D = w I;  b_k = w u_k;  e = w ((r0 r0 + r1 r1) + r2 r2)
//              plane:  D_kl = w (n_k n_l), D_kk = w (n_k n_k + pw);  nu = (n0 u0 + n1 u1) + n2 u2;  b_k = w (n_k nu + pw u_k);
//                      nr = (n0 r0 + n1 r1) + n2 r2;  e = w (nr nr + pw ((r0 r0 + r1 r1) + r2 r2))
//              not live: D, b, e = 0.  handle weight h > 0:  D_kk += h,  b_k += h ((double)p_k - (double)v_k)
//              minv_k = 1 / (D_kk + alpha deg) where that is > 0, else 0
//   matvec   s = 0.0; s += p_j over nbr[offsets[i] .. offsets[i + 1]) in that order;  q_k = Dp_k + alpha (deg p_k - s_k) with
//            Dp_0 = (D00 p0 + D01 p1) + D02 p2, Dp_1 = (D01 p0 + D11 p1) + D12 p2, Dp_2 = (D02 p0 + D12 p1) + D22 p2
//   dot      term_i = (a0 b0 + a1 b1) + a2 b2, summed as mofa_icp_reduce sums a one-column matrix (first level here, fused into the
//            kernel that produces the vectors; upper levels by mofa_icp_reduce)
//   solve    r = b - A x, z = minv r, p = z;  per step: q = A p, a = rho / (p . q), x += a p, r -= a q, z = minv r, rho' = r . z,
//            p = z + (rho' / rho) p;  frozen (rho <= tol^2 rho0, or p . q > 0 false): no vector is written any more.
//
// The as-rigid-as-possible stiffness (mesh.warp(stiffness_model="arap"), mesh.deform) keeps that matrix and changes the right-hand side:
//   rotations  S_ab = 0.0 + e_a e'_b over the list (e = v_i - v_j, e' = e + (d_i - d_j));  Horn's symmetric 4 x 4 matrix of S;  its eigenvector
//              of the largest eigenvalue by MOFA_WARP_JACOBI_SWEEPS cyclic Jacobi sweeps;  R_i the rotation of that unit quaternion;
//              fit_i = sum_j |e' - R_i e|^2.  A non-finite S or R gives the identity and fit 0, counted.
//   arap_rhs   g_c = 0.0 + (0.5 ((Rs_c0 e_0 + Rs_c1 e_1) + Rs_c2 e_2) - e_c) over the list with Rs = R_i + R_j;  b_c = b_c + alpha g_c
// Every index into the two 4 x 4 matrices is a compile-time constant (the pairs are template arguments), so they live in registers.
#include <math.h>

#include "mofa_common.h"

namespace mofa {
namespace {

constexpr long long kWarpMaxIndex = (1ll << 31) - 1;     // V, E, F: int32 indices
constexpr int kWarpChunk = MOFA_ICP_CHUNK;               // 1024 rows per workgroup: 4 per thread, a fixed trip count
constexpr int kWarpMaxSteps = MOFA_WARP_MAX_CG;

__device__ __forceinline__ bool warp_in_range(int v, long long n) { return v >= 0 && (long long)v < n; }

struct WarpGraph {
    const int64_t* offsets;     // [V + 1]
    const int* nbr;             // [E]
    long long V, E;
};

// the list of vertex i, checked: false when it does not lie in [0, E)
__device__ __forceinline__ bool warp_list(const WarpGraph& g, long long i, long long& k0, long long& k1) {
    k0 = g.offsets[i], k1 = g.offsets[i + 1];
    return k0 >= 0 && k1 >= k0 && k1 <= g.E;
}

__global__ __launch_bounds__(256) void k_warp_apply(const float* __restrict__ v, const double* __restrict__ d, long long n3,
                                                    float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    out[i] = (float)((double)v[i] + d[i]);
}

struct WarpSystem {
    const float* verts;         // v [V,3]
    const float* moved;         // y [V,3]
    const float* target;        // c [V,3]
    const float* normals;       // [V,3], or NULL: the normal of face[i]
    const int* face;            // [V], or NULL with `normals`
    const float* tverts;        // the target mesh [TV,3]
    const int* tfaces;          // [TF,3]
    const double* weight;       // [V]
    const double* hweight;      // [V], or NULL
    const float* hpos;          // [V,3], with hweight
    long long TV, TF;
    double pw, alpha;
};

template <int PLANE>
__global__ __launch_bounds__(256) void k_warp_system(WarpSystem in, WarpGraph g, double* __restrict__ D, double* __restrict__ b,
                                                     double* __restrict__ minv, double* __restrict__ energy, int64_t* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int is_bad = 0;
    if (i < g.V) {
        double Dm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // xx xy xz yy yz zz
        double bv[3] = {0.0, 0.0, 0.0};
        double e = 0.0;
        const double w = in.weight[i];
        bool live = w > 0.0;
        double n[3] = {0.0, 0.0, 0.0};
        if (PLANE && live) {
            if (in.face) {
                const int f = in.face[i];
                live = warp_in_range(f, in.TF);
                if (live) {
                    const int ia = in.tfaces[(long long)f * 3 + 0], ib = in.tfaces[(long long)f * 3 + 1], ic = in.tfaces[(long long)f * 3 + 2];
                    live = warp_in_range(ia, in.TV) && warp_in_range(ib, in.TV) && warp_in_range(ic, in.TV);
                    if (live) {
                        double a[3], ab[3], ac[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            a[k] = (double)in.tverts[(long long)ia * 3 + k];
                            ab[k] = (double)in.tverts[(long long)ib * 3 + k] - a[k];
                            ac[k] = (double)in.tverts[(long long)ic * 3 + k] - a[k];
                        }
                        const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
                        const double len = sqrt((cx * cx + cy * cy) + cz * cz);
                        n[0] = cx / len, n[1] = cy / len, n[2] = cz / len;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = (double)in.normals[i * 3 + k];
            }
        }
        double vi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) vi[k] = (double)in.verts[i * 3 + k];
        if (live) {
            double u[3], r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double c = (double)in.target[i * 3 + k];
                u[k] = c - vi[k];
                r[k] = (double)in.moved[i * 3 + k] - c;
            }
            const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            if (PLANE) {
                Dm[0] = w * (n[0] * n[0] + in.pw), Dm[1] = w * (n[0] * n[1]), Dm[2] = w * (n[0] * n[2]);
                Dm[3] = w * (n[1] * n[1] + in.pw), Dm[4] = w * (n[1] * n[2]), Dm[5] = w * (n[2] * n[2] + in.pw);
                const double nu = (n[0] * u[0] + n[1] * u[1]) + n[2] * u[2];
                const double nr = (n[0] * r[0] + n[1] * r[1]) + n[2] * r[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) bv[k] = w * (n[k] * nu + in.pw * u[k]);
                e = w * (nr * nr + in.pw * rr);
            } else {
                Dm[0] = w, Dm[3] = w, Dm[5] = w;
#pragma unroll
                for (int k = 0; k < 3; ++k) bv[k] = w * u[k];
                e = w * rr;
            }
        }
        if (in.hweight) {
            const double h = in.hweight[i];
            if (h > 0.0) {
                Dm[0] += h, Dm[3] += h, Dm[5] += h;
#pragma unroll
                for (int k = 0; k < 3; ++k) bv[k] += h * ((double)in.hpos[i * 3 + k] - vi[k]);
            }
        }
        long long k0, k1;
        const bool ok = warp_list(g, i, k0, k1);
        is_bad = !ok;
        const double ad = in.alpha * (double)(ok ? k1 - k0 : 0);
        const double m[3] = {Dm[0] + ad, Dm[3] + ad, Dm[5] + ad};
#pragma unroll
        for (int k = 0; k < 6; ++k) D[i * 6 + k] = Dm[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b[i * 3 + k] = bv[k];
            minv[i * 3 + k] = (ok && m[k] > 0.0) ? 1.0 / m[k] : 0.0;
        }
        energy[i] = e;
    }
    const int n_bad = __syncthreads_count(is_bad);
    if (threadIdx.x == 0) bad[blockIdx.x] = n_bad;
}

// the tree over the workgroup's 256 partial sums (mofa_icp_reduce's, one column); thread 0 writes the chunk's sum
__device__ __forceinline__ void warp_tree(double acc, double* __restrict__ out) {
    __shared__ double sm[256];
    const int t = threadIdx.x;
    sm[t] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) sm[t] += sm[t + w];
        __syncthreads();
    }
    if (t == 0) *out = sm[0];
}

// q_i = D_i p_i + alpha (deg_i p_i - s_i); false (nothing computed) for a bad list or neighbour
__device__ __forceinline__ bool warp_row(const double* __restrict__ D, const double* __restrict__ p, const WarpGraph& g, double alpha, long long i,
                                         double (&pi)[3], double (&q)[3]) {
    long long k0, k1;
    if (!warp_list(g, i, k0, k1)) return false;
    double s[3] = {0.0, 0.0, 0.0};
    for (long long k = k0; k < k1; ++k) {
        const int j = g.nbr[k];
        if (!warp_in_range(j, g.V)) return false;
        s[0] += p[(long long)j * 3 + 0], s[1] += p[(long long)j * 3 + 1], s[2] += p[(long long)j * 3 + 2];
    }
    pi[0] = p[i * 3 + 0], pi[1] = p[i * 3 + 1], pi[2] = p[i * 3 + 2];
    const double* Di = D + i * 6;
    const double deg = (double)(k1 - k0);
    q[0] = ((Di[0] * pi[0] + Di[1] * pi[1]) + Di[2] * pi[2]) + alpha * (deg * pi[0] - s[0]);
    q[1] = ((Di[1] * pi[0] + Di[3] * pi[1]) + Di[4] * pi[2]) + alpha * (deg * pi[1] - s[1]);
    q[2] = ((Di[2] * pi[0] + Di[4] * pi[1]) + Di[5] * pi[2]) + alpha * (deg * pi[2] - s[2]);
    return true;
}

// record of a solve (doubles, DEVICE): the header's MOFA_WARP_REC_* slots, then rho after 0 .. K steps
__device__ __forceinline__ bool warp_frozen(const double* rec) { return rec && rec[MOFA_WARP_REC_FROZEN] != 0.0; }

__global__ __launch_bounds__(256) void k_warp_matvec(const double* __restrict__ D, const double* __restrict__ p, WarpGraph g, double alpha,
                                                     double* __restrict__ q, double* __restrict__ partial, int64_t* __restrict__ bad,
                                                     const double* __restrict__ rec) {
    if (warp_frozen(rec)) return;
    const long long c0 = (long long)blockIdx.x * kWarpChunk;
    double acc = 0.0;
    int n_bad = 0;
#pragma unroll 1
    for (int k = 0; k < kWarpChunk / 256; ++k) {
        const long long i = c0 + threadIdx.x + (long long)k * 256;
        int is_bad = 0;
        if (i < g.V) {
            double pi[3], qi[3];
            if (warp_row(D, p, g, alpha, i, pi, qi)) {
                q[i * 3 + 0] = qi[0], q[i * 3 + 1] = qi[1], q[i * 3 + 2] = qi[2];
                acc += (pi[0] * qi[0] + pi[1] * qi[1]) + pi[2] * qi[2];
            } else {
                is_bad = 1;
            }
        }
        n_bad += __syncthreads_count(is_bad);
    }
    if (threadIdx.x == 0) bad[blockIdx.x] = n_bad;
    warp_tree(acc, partial + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_warp_dot(const double* __restrict__ a, const double* __restrict__ b, long long V,
                                                  double* __restrict__ partial) {
    const long long c0 = (long long)blockIdx.x * kWarpChunk;
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < kWarpChunk / 256; ++k) {
        const long long i = c0 + threadIdx.x + (long long)k * 256;
        if (i < V) acc += (a[i * 3 + 0] * b[i * 3 + 0] + a[i * 3 + 1] * b[i * 3 + 1]) + a[i * 3 + 2] * b[i * 3 + 2];
    }
    warp_tree(acc, partial + blockIdx.x);
}

// r = b - q, z = minv r, p = z; the first level of r . z
__global__ __launch_bounds__(256) void k_warp_cg_init(const double* __restrict__ b, const double* __restrict__ q, const double* __restrict__ minv,
                                                      long long V, double* __restrict__ r, double* __restrict__ z, double* __restrict__ p,
                                                      double* __restrict__ partial) {
    const long long c0 = (long long)blockIdx.x * kWarpChunk;
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < kWarpChunk / 256; ++k) {
        const long long i = c0 + threadIdx.x + (long long)k * 256;
        if (i < V) {
            double ri[3], zi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ri[c] = b[i * 3 + c] - q[i * 3 + c];
                zi[c] = minv[i * 3 + c] * ri[c];
                r[i * 3 + c] = ri[c], z[i * 3 + c] = zi[c], p[i * 3 + c] = zi[c];
            }
            acc += (ri[0] * zi[0] + ri[1] * zi[1]) + ri[2] * zi[2];
        }
    }
    warp_tree(acc, partial + blockIdx.x);
}

// x += a p, r -= a q, z = minv r; the first level of r . z
__global__ __launch_bounds__(256) void k_warp_cg_update(const double* __restrict__ p, const double* __restrict__ q, const double* __restrict__ minv,
                                                        long long V, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                        double* __restrict__ partial, const double* __restrict__ rec) {
    if (warp_frozen(rec)) return;
    const double a = rec[MOFA_WARP_REC_A];
    const long long c0 = (long long)blockIdx.x * kWarpChunk;
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < kWarpChunk / 256; ++k) {
        const long long i = c0 + threadIdx.x + (long long)k * 256;
        if (i < V) {
            double ri[3], zi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[i * 3 + c] += a * p[i * 3 + c];
                ri[c] = r[i * 3 + c] - a * q[i * 3 + c];
                zi[c] = minv[i * 3 + c] * ri[c];
                r[i * 3 + c] = ri[c], z[i * 3 + c] = zi[c];
            }
            acc += (ri[0] * zi[0] + ri[1] * zi[1]) + ri[2] * zi[2];
        }
    }
    warp_tree(acc, partial + blockIdx.x);
}

// p = z + (rho' / rho) p
__global__ __launch_bounds__(256) void k_warp_cg_direction(const double* __restrict__ z, long long n3, double* __restrict__ p,
                                                           const double* __restrict__ rho_new, const double* __restrict__ rec, int step) {
    if (warp_frozen(rec)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const double beta = *rho_new / rec[MOFA_WARP_REC_RHO + step];
    p[i] = z[i] + beta * p[i];
}

__global__ void k_warp_cg_clear(double* __restrict__ rec, int n, double tol2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) rec[i] = i == MOFA_WARP_REC_TOL2 ? tol2 : 0.0;
}

// the one thread of step `step`: records rho, decides the freeze, leaves a; step == K only records
__global__ void k_warp_cg_scalar(double* __restrict__ rec, const double* __restrict__ rho_in, const double* __restrict__ pq_in, int step, int K) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double rho = *rho_in;
    rec[MOFA_WARP_REC_RHO + step] = rho;
    if (step >= K) return;
    if (rec[MOFA_WARP_REC_FROZEN] == 0.0) {
        const double pq = *pq_in;
        if (rho <= rec[MOFA_WARP_REC_TOL2] * rec[MOFA_WARP_REC_RHO]) {
            rec[MOFA_WARP_REC_FROZEN] = 1.0, rec[MOFA_WARP_REC_CAUSE] = (double)MOFA_WARP_STOP_TOLERANCE;
        } else if (!(pq > 0.0)) {
            rec[MOFA_WARP_REC_FROZEN] = 1.0, rec[MOFA_WARP_REC_CAUSE] = (double)MOFA_WARP_STOP_BREAKDOWN;
        } else {
            rec[MOFA_WARP_REC_A] = rho / pq;
            rec[MOFA_WARP_REC_STEPS] = (double)(step + 1);
            return;
        }
    }
    rec[MOFA_WARP_REC_A] = 0.0;
}

// one Jacobi rotation in the plane (P, Q) of the symmetric matrix a (both triangles kept) and of the eigenvector matrix v; the header's order
template <int P, int Q>
__device__ __forceinline__ void warp_jacobi_pair(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq != 0.0) {
        const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        a[P][P] = a[P][P] - t * apq, a[Q][Q] = a[Q][Q] + t * apq;
        a[P][Q] = 0.0, a[Q][P] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k != P && k != Q) {
                const double akp = a[k][P], akq = a[k][Q];
                a[k][P] = a[P][k] = c * akp - s * akq;
                a[k][Q] = a[Q][k] = s * akp + c * akq;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double vkp = v[k][P], vkq = v[k][Q];
            v[k][P] = c * vkp - s * vkq;
            v[k][Q] = s * vkp + c * vkq;
        }
    }
}

// the rotation (row-major) that best takes the rest edges of a neighbourhood onto the deformed ones, from their covariance S (finite);
// false when an entry of it is not finite
__device__ __forceinline__ bool warp_fit_rotation(const double (&S)[3][3], double (&R)[9]) {
    double a[4][4], v[4][4];
    a[0][0] = (S[0][0] + S[1][1]) + S[2][2], a[0][1] = S[1][2] - S[2][1], a[0][2] = S[2][0] - S[0][2], a[0][3] = S[0][1] - S[1][0];
    a[1][1] = (S[0][0] - S[1][1]) - S[2][2], a[1][2] = S[0][1] + S[1][0], a[1][3] = S[2][0] + S[0][2];
    a[2][2] = (S[1][1] - S[0][0]) - S[2][2], a[2][3] = S[1][2] + S[2][1];
    a[3][3] = (S[2][2] - S[0][0]) - S[1][1];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < p) a[p][q] = a[q][p];
            v[p][q] = p == q ? 1.0 : 0.0;
        }
    }
#pragma unroll 1
    for (int sweep = 0; sweep < MOFA_WARP_JACOBI_SWEEPS; ++sweep) {      // (rolled: the sweep indexes nothing)
        warp_jacobi_pair<0, 1>(a, v), warp_jacobi_pair<0, 2>(a, v), warp_jacobi_pair<0, 3>(a, v);
        warp_jacobi_pair<1, 2>(a, v), warp_jacobi_pair<1, 3>(a, v), warp_jacobi_pair<2, 3>(a, v);
    }
    // the column of the largest diagonal entry, the lowest index among equal ones
    double best = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
    for (int m = 1; m < 4; ++m) {                                       // (selects of values: a branch here would keep v in memory)
        const bool larger = a[m][m] > best;
        const double c0 = v[0][m], c1 = v[1][m], c2 = v[2][m], c3 = v[3][m];
        best = larger ? a[m][m] : best;
        q0 = larger ? c0 : q0, q1 = larger ? c1 : q1, q2 = larger ? c2 : q2, q3 = larger ? c3 : q3;
    }
    const double n = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double w = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = 1.0 - 2.0 * (x * x + y * y);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite &= (bool)isfinite(R[k]);
    return finite;
}

__global__ __launch_bounds__(256) void k_warp_rotations(const float* __restrict__ verts, const double* __restrict__ disp, WarpGraph g,
                                                        double* __restrict__ R, double* __restrict__ fit, int64_t* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int is_bad = 0, is_odd = 0;
    if (i < g.V) {
        double Ri[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        double f = 0.0;
        double vi[3], di[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) vi[c] = (double)verts[i * 3 + c], di[c] = disp[i * 3 + c];
        long long k0, k1;
        bool ok = warp_list(g, i, k0, k1);
        double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        if (ok) {
            for (long long k = k0; k < k1; ++k) {
                const int j = g.nbr[k];
                if (!warp_in_range(j, g.V)) {
                    ok = false;
                    break;
                }
                double e[3], ep[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    e[c] = vi[c] - (double)verts[(long long)j * 3 + c];
                    ep[c] = e[c] + (di[c] - disp[(long long)j * 3 + c]);
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int b = 0; b < 3; ++b) S[a][b] += e[a] * ep[b];
                }
            }
        }
        if (!ok) {
            is_bad = 1;
        } else {
            bool finite = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) finite &= (bool)isfinite(S[a][b]);
            }
            double Rq[9];
            if (finite) finite = warp_fit_rotation(S, Rq);
            if (!finite) {
                is_odd = 1;
            } else {
#pragma unroll
                for (int c = 0; c < 9; ++c) Ri[c] = Rq[c];
                for (long long k = k0; k < k1; ++k) {
                    const long long j = g.nbr[k];
                    double e[3], r[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) e[c] = vi[c] - (double)verts[j * 3 + c];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double ep = e[c] + (di[c] - disp[j * 3 + c]);
                        r[c] = ep - ((Ri[3 * c] * e[0] + Ri[3 * c + 1] * e[1]) + Ri[3 * c + 2] * e[2]);
                    }
                    f += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) R[i * 9 + c] = Ri[c];
        fit[i] = f;
    }
    const int n_bad = __syncthreads_count(is_bad);
    const int n_odd = __syncthreads_count(is_odd);
    if (threadIdx.x == 0) bad[(long long)blockIdx.x * 2] = n_bad, bad[(long long)blockIdx.x * 2 + 1] = n_odd;
}

__global__ __launch_bounds__(256) void k_warp_arap_rhs(const float* __restrict__ verts, const double* __restrict__ R, WarpGraph g, double alpha,
                                                       double* __restrict__ b, int64_t* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int is_bad = 0;
    if (i < g.V) {
        long long k0, k1;
        bool ok = warp_list(g, i, k0, k1);
        double gi[3] = {0.0, 0.0, 0.0};
        if (ok) {
            double vi[3], Ri[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) vi[c] = (double)verts[i * 3 + c];
#pragma unroll
            for (int c = 0; c < 9; ++c) Ri[c] = R[i * 9 + c];
            for (long long k = k0; k < k1; ++k) {
                const int j = g.nbr[k];
                if (!warp_in_range(j, g.V)) {
                    ok = false;
                    break;
                }
                double e[3], Rs[9];
#pragma unroll
                for (int c = 0; c < 3; ++c) e[c] = vi[c] - (double)verts[(long long)j * 3 + c];
#pragma unroll
                for (int c = 0; c < 9; ++c) Rs[c] = Ri[c] + R[(long long)j * 9 + c];
#pragma unroll
                for (int c = 0; c < 3; ++c) gi[c] += 0.5 * ((Rs[3 * c] * e[0] + Rs[3 * c + 1] * e[1]) + Rs[3 * c + 2] * e[2]) - e[c];
            }
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) b[i * 3 + c] = b[i * 3 + c] + alpha * gi[c];
        } else {
            is_bad = 1;
        }
    }
    const int n_bad = __syncthreads_count(is_bad);
    if (threadIdx.x == 0) bad[blockIdx.x] = n_bad;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// the levels of a sum over V rows: n[0] = ceil(V / 1024) first-level sums, n[l + 1] = ceil(n[l] / 1024) until one is left
inline int warp_levels(long long V, long long (&n)[4]) {
    int L = 0;
    long long m = V;
    do {
        m = (m + kWarpChunk - 1) / kWarpChunk;
        n[L++] = m;
    } while (m > 1 && L < 4);
    return L;
}

inline long long warp_level_doubles(long long V) {
    long long n[4], total = 0;
    const int L = warp_levels(V, n);
    for (int l = 0; l < L; ++l) total += n[l];
    return total;
}

}  // namespace
}  // namespace mofa

using namespace mofa;

#define MOFA_WARP_COUNT(what, name, n) MOFA_REQUIRE((n) >= 1 && (n) <= kWarpMaxIndex, what ": " name " = %lld (want 1 .. 2^31 - 1)", (long long)(n))

static int warp_graph(const char* what, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, WarpGraph& g) {
    MOFA_REQUIRE(offsets, "%s: null pointer", what);
    MOFA_REQUIRE(V >= 1 && V <= kWarpMaxIndex, "%s: V = %lld (want 1 .. 2^31 - 1)", what, (long long)V);
    MOFA_REQUIRE(E >= 0 && E <= kWarpMaxIndex, "%s: E = %lld (want 0 .. 2^31 - 1)", what, (long long)E);
    MOFA_REQUIRE(nbr || E == 0, "%s: null neighbours with E = %lld", what, (long long)E);
    g.offsets = offsets, g.nbr = nbr, g.V = V, g.E = E;
    return MOFA_OK;
}

// the upper levels of a sum whose first level lies in `levels` (n[0] numbers); returns where the one number left is
static int warp_reduce_up(double* levels, long long V, const double** result, void* stream) {
    long long n[4];
    const int L = warp_levels(V, n);
    double* at = levels;
    for (int l = 0; l + 1 < L; ++l) {
        if (int rc = mofa_icp_reduce(at, n[l], 1, at + n[l], stream)) return rc;
        at += n[l];
    }
    *result = at;
    return MOFA_OK;
}

extern "C" {

int mofa_warp_apply(const float* verts, const double* disp, int64_t V, float* out, void* stream) {
    MOFA_REQUIRE(verts && disp && out, "warp_apply: null pointer");
    MOFA_WARP_COUNT("warp_apply", "V", V);
    hipLaunchKernelGGL(k_warp_apply, dim3(blocks_of(3 * (long long)V, 256)), dim3(256), 0, (hipStream_t)stream, verts, disp, 3 * (long long)V, out);
    return check_launch("k_warp_apply");
}

int mofa_warp_system(const float* verts, const float* moved, const float* target, const float* normals, const int32_t* face, const float* tverts,
                     int64_t TV, const int32_t* tfaces, int64_t TF, const double* weight, const double* handle_weight, const float* handle_pos,
                     const int64_t* offsets, int64_t E, int64_t V, int32_t metric, double point_weight, double alpha, double* D, double* b,
                     double* minv, double* energy, int64_t* bad, void* stream) {
    WarpGraph g;
    if (int rc = warp_graph("warp_system", offsets, nullptr, 0, V, g)) return rc;
    MOFA_REQUIRE(E >= 0 && E <= kWarpMaxIndex, "warp_system: E = %lld (want 0 .. 2^31 - 1)", (long long)E);
    g.E = E;
    MOFA_REQUIRE(verts && moved && target && weight && D && b && minv && energy && bad, "warp_system: null pointer");
    MOFA_REQUIRE(metric == MOFA_ICP_POINT || metric == MOFA_ICP_PLANE, "warp_system: metric = %d (want MOFA_ICP_POINT or MOFA_ICP_PLANE)", (int)metric);
    if (metric == MOFA_ICP_PLANE) {
        MOFA_REQUIRE((face != nullptr) != (normals != nullptr), "warp_system: the plane metric takes the closest faces or explicit normals, one of the two");
        if (face) {
            MOFA_REQUIRE(tverts && tfaces, "warp_system: null target mesh");
            MOFA_REQUIRE(TV >= 1 && TV <= kWarpMaxIndex && TF >= 1 && TF <= kWarpMaxIndex, "warp_system: TV = %lld, TF = %lld (want 1 .. 2^31 - 1)",
                         (long long)TV, (long long)TF);
        }
    }
    MOFA_REQUIRE((handle_weight != nullptr) == (handle_pos != nullptr), "warp_system: handle weights and positions come together");
    MOFA_REQUIRE(point_weight >= 0.0 && isfinite(point_weight), "warp_system: point_weight = %g (want finite, >= 0)", point_weight);
    MOFA_REQUIRE(alpha >= 0.0 && isfinite(alpha), "warp_system: alpha = %g (want finite, >= 0)", alpha);
    WarpSystem in;
    in.verts = verts, in.moved = moved, in.target = target, in.normals = normals, in.face = face, in.tverts = tverts, in.tfaces = tfaces;
    in.weight = weight, in.hweight = handle_weight, in.hpos = handle_pos, in.TV = TV, in.TF = TF, in.pw = point_weight, in.alpha = alpha;
    if (metric == MOFA_ICP_PLANE)
        hipLaunchKernelGGL(k_warp_system<1>, dim3(blocks_of(V, 256)), dim3(256), 0, (hipStream_t)stream, in, g, D, b, minv, energy, bad);
    else
        hipLaunchKernelGGL(k_warp_system<0>, dim3(blocks_of(V, 256)), dim3(256), 0, (hipStream_t)stream, in, g, D, b, minv, energy, bad);
    return check_launch("k_warp_system");
}

int mofa_warp_matvec(const double* D, const double* p, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, double alpha, double* q,
                     double* partial, int64_t* bad, void* stream) {
    WarpGraph g;
    if (int rc = warp_graph("warp_matvec", offsets, nbr, E, V, g)) return rc;
    MOFA_REQUIRE(D && p && q && partial && bad, "warp_matvec: null pointer");
    MOFA_REQUIRE(p != q, "warp_matvec: the product does not run in place (p == q)");
    MOFA_REQUIRE(alpha >= 0.0 && isfinite(alpha), "warp_matvec: alpha = %g (want finite, >= 0)", alpha);
    hipLaunchKernelGGL(k_warp_matvec, dim3(blocks_of(V, kWarpChunk)), dim3(256), 0, (hipStream_t)stream, D, p, g, alpha, q, partial, bad,
                       (const double*)nullptr);
    return check_launch("k_warp_matvec");
}

int mofa_warp_dot(const double* a, const double* b, int64_t V, double* partial, void* stream) {
    MOFA_REQUIRE(a && b && partial, "warp_dot: null pointer");
    MOFA_WARP_COUNT("warp_dot", "V", V);
    hipLaunchKernelGGL(k_warp_dot, dim3(blocks_of(V, kWarpChunk)), dim3(256), 0, (hipStream_t)stream, a, b, (long long)V, partial);
    return check_launch("k_warp_dot");
}

size_t mofa_warp_workspace_doubles(int64_t V) {
    if (V < 1 || V > kWarpMaxIndex) return 0;
    return (size_t)(12 * (long long)V + 2 * warp_level_doubles(V));
}

int mofa_warp_solve(const double* D, const double* b, const double* minv, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V,
                    double alpha, int32_t cg_iterations, double cg_tol, double* x, double* work, double* rec, int64_t* bad, void* stream) {
    WarpGraph g;
    if (int rc = warp_graph("warp_solve", offsets, nbr, E, V, g)) return rc;
    MOFA_REQUIRE(D && b && minv && x && work && rec && bad, "warp_solve: null pointer");
    MOFA_REQUIRE(alpha >= 0.0 && isfinite(alpha), "warp_solve: alpha = %g (want finite, >= 0)", alpha);
    MOFA_REQUIRE(cg_iterations >= 1 && cg_iterations <= kWarpMaxSteps, "warp_solve: cg_iterations = %d (want 1 .. %d)", (int)cg_iterations, kWarpMaxSteps);
    MOFA_REQUIRE(cg_tol >= 0.0 && cg_tol < 1.0, "warp_solve: cg_tol = %g (want in [0, 1))", cg_tol);
    const hipStream_t s = (hipStream_t)stream;
    const long long n3 = 3 * (long long)V, lv = warp_level_doubles(V);
    double *r = work, *z = r + n3, *p = z + n3, *q = p + n3, *pq_levels = q + n3, *rz_levels = pq_levels + lv;
    const unsigned chunks = blocks_of(V, kWarpChunk), flat = blocks_of(n3, 256);
    const int K = cg_iterations, n_rec = MOFA_WARP_REC_RHO + K + 1;
    const double *pq = nullptr, *rz = nullptr;
    hipLaunchKernelGGL(k_warp_cg_clear, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, rec, n_rec, cg_tol * cg_tol);
    if (int rc = check_launch("k_warp_cg_clear")) return rc;
    // r = b - A x, z = minv r, p = z
    hipLaunchKernelGGL(k_warp_matvec, dim3(chunks), dim3(256), 0, s, D, (const double*)x, g, alpha, q, pq_levels, bad, (const double*)nullptr);
    if (int rc = check_launch("k_warp_matvec")) return rc;
    hipLaunchKernelGGL(k_warp_cg_init, dim3(chunks), dim3(256), 0, s, b, (const double*)q, minv, (long long)V, r, z, p, rz_levels);
    if (int rc = check_launch("k_warp_cg_init")) return rc;
    if (int rc = warp_reduce_up(rz_levels, V, &rz, stream)) return rc;
    for (int step = 0; step < K; ++step) {
        hipLaunchKernelGGL(k_warp_matvec, dim3(chunks), dim3(256), 0, s, D, (const double*)p, g, alpha, q, pq_levels, bad, (const double*)rec);
        if (int rc = check_launch("k_warp_matvec")) return rc;
        if (int rc = warp_reduce_up(pq_levels, V, &pq, stream)) return rc;
        hipLaunchKernelGGL(k_warp_cg_scalar, dim3(1), dim3(64), 0, s, rec, rz, pq, step, K);
        if (int rc = check_launch("k_warp_cg_scalar")) return rc;
        hipLaunchKernelGGL(k_warp_cg_update, dim3(chunks), dim3(256), 0, s, (const double*)p, (const double*)q, minv, (long long)V, x, r, z,
                           rz_levels, (const double*)rec);
        if (int rc = check_launch("k_warp_cg_update")) return rc;
        if (int rc = warp_reduce_up(rz_levels, V, &rz, stream)) return rc;
        hipLaunchKernelGGL(k_warp_cg_direction, dim3(flat), dim3(256), 0, s, (const double*)z, n3, p, rz, (const double*)rec, step);
        if (int rc = check_launch("k_warp_cg_direction")) return rc;
    }
    hipLaunchKernelGGL(k_warp_cg_scalar, dim3(1), dim3(64), 0, s, rec, rz, rz, K, K);
    return check_launch("k_warp_cg_scalar");
}

int mofa_warp_rotations(const float* verts, const double* disp, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, double* R,
                        double* fit, int64_t* bad, void* stream) {
    WarpGraph g;
    if (int rc = warp_graph("warp_rotations", offsets, nbr, E, V, g)) return rc;
    MOFA_REQUIRE(verts && disp && R && fit && bad, "warp_rotations: null pointer");
    hipLaunchKernelGGL(k_warp_rotations, dim3(blocks_of(V, 256)), dim3(256), 0, (hipStream_t)stream, verts, disp, g, R, fit, bad);
    return check_launch("k_warp_rotations");
}

int mofa_warp_arap_rhs(const float* verts, const double* R, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, double alpha,
                       double* b, int64_t* bad, void* stream) {
    WarpGraph g;
    if (int rc = warp_graph("warp_arap_rhs", offsets, nbr, E, V, g)) return rc;
    MOFA_REQUIRE(verts && R && b && bad, "warp_arap_rhs: null pointer");
    MOFA_REQUIRE(R != b, "warp_arap_rhs: the rotations and the right-hand side are two buffers (R == b)");
    MOFA_REQUIRE(alpha >= 0.0 && isfinite(alpha), "warp_arap_rhs: alpha = %g (want finite, >= 0)", alpha);
    hipLaunchKernelGGL(k_warp_arap_rhs, dim3(blocks_of(V, 256)), dim3(256), 0, (hipStream_t)stream, verts, R, g, alpha, b, bad);
    return check_launch("k_warp_arap_rhs");
}

}  // extern "C"
