// Dense real symmetric / complex Hermitian eigensolver (gfx950): all or a selected range of the
// eigenvalues, and an orthonormal set of eigenvectors, of A (n x n, EIGSOL_F64 / EIGSOL_C128).
//
//   a. the largest modulus in the lower triangle is found (eigh_absmax) and, only where it lies outside
//      [2^-410, 2^410], the triangle is multiplied by the power of two that brings it into [1, 2)
//      (eigh_rescale; dsyevx's scaling, exact here): the squares the later steps form (Householder norms, e^2
//      in the Sturm count and the split rule, the norm of an iterate) then neither overflow nor underflow.
//      Only the returned eigenvalues and the comparison with a value range are scaled back.  Then the lower
//      triangle is mirrored on the device (eigh_symmetrise), so the matrix reduced is Hermitian;
//   b. hessenberg_blocked<S> (hessenberg.hip) reduces it; on a Hermitian matrix H is tridiagonal, and the
//      reduction keeps every panel's V and T;
//   c. d_i = Re h_ii, e_i = |h_{i+1,i}| and the phases h_{i+1,i} / |h_{i+1,i}| (eigh_extract); the host
//      accumulates the unitary diagonal D (D_0 = 1, D_{i+1} = D_i phase_i), so D^H H D = T is real with
//      non-negative off-diagonals;
//   d. T splits into blocks where |e_i| <= eps sqrt(|d_i| |d_{i+1}|) or e_i^2 <= safemin (tridiag_plan, host);
//   e. every eigenvalue of every block of order >= 2 by bisection on the Sturm count, one lane per
//      eigenvalue, d and e^2 staged through LDS in chunks (eigh_bisect); a 1 x 1 block's eigenvalue is its
//      entry.  The selection (all / index range / half-open value range) is taken from the sorted values,
//      so a selected run returns bitwise the values of a full run;
//   f. eigenvectors of T by dstein's scheme: inverse iteration on the partial-pivot LU of T_block - lambda I
//      from a counter-based pseudo-random start, close eigenvalues perturbed apart, Gram-Schmidt against
//      the finished vectors of the same cluster after every solve, stopped by the growth test (at most 5
//      iterations; failures are counted).  One workgroup owns one cluster (eigh_stein): the serial
//      recurrences of the factorisation and the solves take their operands 64 at a time from wave 0's
//      registers, the scalings, dots and updates run on all threads;
//   g. Z = Q (D Z_T) with the stored panels, three MFMA GEMMs per panel (hess_backtransform), and each
//      column's phase fixed so that its largest-modulus component (the first on ties) is real positive.
// Under EIGSOL_EIGH_METHOD_DC steps e and f are replaced by divide and conquer on T (eigh_dc.hip): all eigenpairs
// of T, the selection taken from the sorted values and the matching columns.
// No floating-point atomics; every sum has a fixed order, so two runs give the same bits.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>

#include "cholesky.hpp"
#include "kernels_common.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

constexpr double kEps = DBL_EPSILON;   // dlamch('P')
constexpr double kSafeMin = DBL_MIN;   // dlamch('S')

__device__ __forceinline__ double conj_s(double a) { return a; }
__device__ __forceinline__ cplx conj_s(cplx a) { return cplx{a.re, -a.im}; }

// upper triangle <- conj of the lower one; the diagonal's imaginary part dropped
template <class S>
__global__ __launch_bounds__(256) void eigh_symmetrise(S* A, int n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int i = (int)(idx % n);
    const int64_t j = idx / n;
    if (i < j) A[i + j * n] = conj_s(A[j + (int64_t)i * n]);
    else if (i == j) {
        S v = A[idx];
        set_re_im(v, *reinterpret_cast<const double*>(&v), 0.0);
        A[idx] = v;
    }
}

// ------------------------------------------------------------------ scaling
constexpr int kAbsmaxBlocks = 256;    // partial maxima, reduced again by every block of eigh_rescale
constexpr int kRescaleBlocks = 1024;
constexpr double kScaleMin = 0x1p-410, kScaleMax = 0x1p410;   // the range taken as it is

__device__ __forceinline__ double absmax_of(double a, bool /*diag*/) { return fabs(a); }
__device__ __forceinline__ double absmax_of(cplx a, bool diag) { return diag ? fabs(a.re) : fmax(fabs(a.re), fabs(a.im)); }
__device__ __forceinline__ double scale_by(double a, int k) { return ldexp(a, k); }
__device__ __forceinline__ cplx scale_by(cplx a, int k) { return cplx{ldexp(a.re, k), ldexp(a.im, k)}; }

// max of 256 threads' values (a maximum does not depend on the order it is taken in)
__device__ __forceinline__ double block_max_256(double v, double* sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    return sm[0];
}

// partial[blockIdx.x] = max over this block's share of the lower triangle of |re|, |im| (the diagonal's
// imaginary part is not part of the matrix).  fmax drops a NaN: the reduction reports it, as before.
template <class S>
__global__ __launch_bounds__(256) void eigh_absmax(const S* A, int n, double* partial) {
    __shared__ double sm[256];
    const int64_t nn = (int64_t)n * n;
    double v = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nn; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx % n, j = idx / n;
        if (i >= j) v = fmax(v, absmax_of(A[idx], i == j));
    }
    v = block_max_256(v, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// The exponent k (A <- 2^k A): 0 inside [kScaleMin, kScaleMax], and for a zero or a non-finite maximum.
__device__ __forceinline__ int scale_exponent(double amax) {
    if (!(amax > 0.0) || isinf(amax) || (amax >= kScaleMin && amax <= kScaleMax)) return 0;
    return -ilogb(amax);
}

// Every block takes the maximum of the np <= 256 partial maxima and the exponent from it; where that is not
// zero the lower triangle is scaled (exactly: ldexp).  *kexp receives the exponent.
template <class S>
__global__ __launch_bounds__(256) void eigh_rescale(S* A, int n, const double* partial, int np, int* kexp) {
    __shared__ double sm[256];
    const double amax = block_max_256((int)threadIdx.x < np ? partial[threadIdx.x] : 0.0, sm);
    const int k = scale_exponent(amax);
    if (blockIdx.x == 0 && threadIdx.x == 0) *kexp = k;
    if (k == 0) return;
    const int64_t nn = (int64_t)n * n;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nn; idx += (int64_t)gridDim.x * 256)
        if (idx % n >= idx / n) A[idx] = scale_by(A[idx], k);
}

__device__ __forceinline__ void phase_of(double h, double& a, double& ph) {
    a = fabs(h);
    ph = h < 0.0 ? -1.0 : 1.0;
}
__device__ __forceinline__ void phase_of(cplx h, double& a, cplx& ph) {
    a = hypot(h.re, h.im);
    ph = a == 0.0 ? cplx{1.0, 0.0} : cplx{h.re / a, h.im / a};
}

// d_i = Re h_ii, e_i = |h_{i+1,i}|, ph_i = h_{i+1,i} / e_i (1 where e_i = 0)
template <class S>
__global__ __launch_bounds__(256) void eigh_extract(const S* H, int n, double* d, double* e, S* ph) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    d[i] = *reinterpret_cast<const double*>(&H[i + (int64_t)i * n]);
    if (i + 1 < n) {
        double a;
        S p;
        phase_of(H[(i + 1) + (int64_t)i * n], a, p);
        e[i] = a;
        ph[i] = p;
    }
}

// ------------------------------------------------------------------ bisection
// One wave: up to 64 consecutive eigenvalue indices [k0, k0 + cnt) of the block of rows [b0, b0 + bn).
struct BisectWave {
    int b0, bn, k0, cnt;
    double gl, gu, pivmin;
};
constexpr int kBisectChunk = 1024;   // 2 x 8 KiB of LDS
constexpr int kBisectMaxIter = 1200;

// lambda_k = the smallest x with count(x) >= k + 1, count(x) = #{q_i <= 0}, q_i = d_i - x - e_{i-1}^2 / q_{i-1}
// (dstebz's pivmin guard).  out[b0 + k] receives the k-th smallest eigenvalue of the block.
__global__ __launch_bounds__(64) void eigh_bisect(const double* d, const double* e, const BisectWave* waves, double* out) {
    __shared__ double sd[kBisectChunk], se[kBisectChunk];
    const BisectWave w = waves[blockIdx.x];
    const int lane = threadIdx.x;
    const bool active = lane < w.cnt;
    const int k = w.k0 + lane;
    double lo = w.gl, hi = w.gu;
    for (int it = 0; it < kBisectMaxIter; ++it) {
        const double mid = lo + 0.5 * (hi - lo);
        const bool done = !active || !(lo < mid && mid < hi) ||
                          (hi - lo) <= 2.0 * kEps * fmax(fabs(lo), fabs(hi)) + w.pivmin;
        if (__all(done)) break;
        int cnt = 0;
        double q = 1.0;
        for (int c0 = 0; c0 < w.bn; c0 += kBisectChunk) {
            const int len = min(kBisectChunk, w.bn - c0);
            __syncthreads();
            for (int t = lane; t < len; t += 64) {
                const int g = w.b0 + c0 + t;
                sd[t] = d[g];
                const double ev = (c0 + t) == 0 ? 0.0 : e[g - 1];
                se[t] = ev * ev;
            }
            __syncthreads();
            for (int t = 0; t < len; ++t) {
                q = (sd[t] - se[t] / q) - mid;
                if (fabs(q) < w.pivmin) q = -w.pivmin;
                cnt += q <= 0.0 ? 1 : 0;
            }
        }
        if (!done) {
            if (cnt >= k + 1) hi = mid;
            else lo = mid;
        }
    }
    if (active) out[w.b0 + k] = lo + 0.5 * (hi - lo);
}

// ------------------------------------------------------------------ inverse iteration
// One cluster: `cnt` selected eigenvalues (columns items[first .. first + cnt) of Z_T, ascending) of the
// block of rows [b0, b0 + bn) whose 1-norm is onenrm.
struct SteinCluster {
    int b0, bn, first, cnt;
    double onenrm;
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform on (-1, 1), a function of (block start, eigenvalue index in the block, row) only
__device__ __forceinline__ double start_entry(int b0, int k, int i) {
    const uint64_t h = mix64(mix64(((uint64_t)(uint32_t)b0 << 32) | (uint32_t)k) + (uint64_t)i);
    return ((double)(h >> 11) + 0.5) * (2.0 / 9007199254740992.0) - 1.0;
}

// The factorisation and the solves are serial recurrences.  The whole wave runs them: 64 consecutive
// entries of every operand are loaded at once (one coalesced load each), a step takes its entries from the
// lane that holds them (v_readlane), every lane carries the same scalars, lane t keeps step t's results, and
// 64 results go back in one store.  The arithmetic is that of a single lane walking the arrays.
__device__ __forceinline__ double lane_value(double v, int t) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), t);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), t);
    return __hiloint2double(hi, lo);
}

// dlagtf with tol = 0 on T - lambda I already formed in a (diagonal), b (super-), c (sub-diagonal);
// d2 receives the second super-diagonal, in the pivot flags (in[n - 1]: the first tiny pivot, 1-based).
// Called by all 64 lanes; n >= 2.
__device__ void tri_lu_factor(int n, double* a, double* b, double* c, double* d2, double* in, int lane) {
    const double tl = kEps;
    double last = 0.0;
    double ak = a[0], bk = b[0];
    double scale1 = fabs(ak) + fabs(bk);
    for (int base = 0; base < n - 1; base += 64) {
        const int idx = base + lane;
        const int cnt = min(64, n - 1 - base);
        const double a1 = idx + 1 < n ? a[idx + 1] : 0.0;       // a[k + 1], as stored
        const double c0 = idx < n - 1 ? c[idx] : 0.0;           // c[k]
        const double b1 = idx + 1 < n - 1 ? b[idx + 1] : 0.0;   // b[k + 1] (k < n - 2)
        double oa = 0.0, ob = 0.0, oc = 0.0, od = 0.0, oi = 0.0;
        for (int t = 0; t < cnt; ++t) {
            const int k = base + t;
            double ak1 = lane_value(a1, t);
            const double ck = lane_value(c0, t);
            const double bk1 = lane_value(b1, t);
            double scale2 = fabs(ck) + fabs(ak1);
            if (k < n - 2) scale2 += fabs(bk1);
            const double piv1 = ak == 0.0 ? 0.0 : fabs(ak) / scale1;
            double piv2 = 0.0;
            double nbk1 = bk1;
            double va = ak, vb = bk, vc = ck, vd = 0.0, vi = 0.0;
            if (ck == 0.0) {
                scale1 = scale2;
            } else {
                piv2 = fabs(ck) / scale2;
                if (piv2 <= piv1) {
                    scale1 = scale2;
                    const double mult = ck / ak;
                    vc = mult;
                    ak1 = ak1 - mult * bk;
                } else {
                    vi = 1.0;
                    const double mult = ak / ck;
                    va = ck;
                    const double temp = ak1;
                    ak1 = bk - mult * temp;
                    if (k < n - 2) {
                        vd = bk1;
                        nbk1 = -mult * bk1;
                    }
                    vb = temp;
                    vc = mult;
                }
            }
            if (fmax(piv1, piv2) <= tl && last == 0.0) last = (double)(k + 1);
            if (lane == t) { oa = va; ob = vb; oc = vc; od = vd; oi = vi; }
            ak = ak1;
            bk = nbk1;
        }
        if (lane < cnt) {
            a[idx] = oa;
            b[idx] = ob;
            c[idx] = oc;
            if (idx < n - 2) d2[idx] = od;
            in[idx] = oi;
        }
    }
    if (fabs(ak) <= scale1 * tl && last == 0.0) last = (double)n;
    if (lane == 0) {
        a[n - 1] = ak;
        in[n - 1] = last;
    }
}

// dlagts, job = -1: (T - lambda I) x = y from tri_lu_factor's factors, tiny pivots perturbed by tol: the
// forward sweep, then (after a barrier: it reads what other lanes stored) the backward one.  Each called by
// all 64 lanes of one wave; n >= 2.
__device__ void tri_lu_forward(int n, const double* c, const double* in, double* y, int lane) {
    double yk = y[0];
    for (int base = 1; base < n; base += 64) {
        const int idx = base + lane;
        const int cnt = min(64, n - base);
        const double yr = idx < n ? y[idx] : 0.0;
        const double cr = idx < n ? c[idx - 1] : 0.0;
        const double ir = idx < n ? in[idx - 1] : 0.0;
        double o = 0.0;
        for (int t = 0; t < cnt; ++t) {
            const double yn = lane_value(yr, t), ck = lane_value(cr, t);
            double out;
            if (lane_value(ir, t) == 0.0) {
                out = yk;
                yk = yn - ck * yk;
            } else {
                out = yn;
                yk = yk - ck * yn;
            }
            if (lane == t) o = out;
        }
        if (lane < cnt) y[idx - 1] = o;
    }
    if (lane == 0) y[n - 1] = yk;
}
__device__ void tri_lu_backward(int n, const double* a, const double* b, const double* d2, double* y, double tol,
                                int lane) {
    const double sfmin = kSafeMin, bignum = 1.0 / kSafeMin;
    double y1 = 0.0, y2 = 0.0;   // x[k + 1], x[k + 2]
    for (int top = n - 1; top >= 0; top -= 64) {
        const int idx = top - lane;   // lane t holds row top - t
        const int cnt = min(64, top + 1);
        const double yr = idx >= 0 ? y[idx] : 0.0;
        const double ar = idx >= 0 ? a[idx] : 1.0;
        const double br = idx >= 0 && idx <= n - 2 ? b[idx] : 0.0;
        const double dr = idx >= 0 && idx <= n - 3 ? d2[idx] : 0.0;
        double o = 0.0;
        for (int t = 0; t < cnt; ++t) {
            const int k = top - t;
            double temp = lane_value(yr, t);
            if (k <= n - 3) temp = temp - lane_value(br, t) * y1 - lane_value(dr, t) * y2;
            else if (k == n - 2) temp = temp - lane_value(br, t) * y1;
            double ak = lane_value(ar, t);
            double pert = ak < 0.0 ? -fabs(tol) : fabs(tol);
            for (int guard = 0; guard < 2200; ++guard) {
                const double absak = fabs(ak);
                if (absak < 1.0) {
                    if (absak < sfmin) {
                        if (absak == 0.0 || fabs(temp) * sfmin > absak) {
                            ak += pert;
                            pert *= 2.0;
                            continue;
                        }
                        temp *= bignum;
                        ak *= bignum;
                    } else if (fabs(temp) > absak * bignum) {
                        ak += pert;
                        pert *= 2.0;
                        continue;
                    }
                }
                break;
            }
            const double xk = temp / ak;
            if (lane == t) o = xk;
            y2 = y1;
            y1 = xk;
        }
        if (lane < cnt) y[idx] = o;
    }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// Workgroup reductions in a fixed order (wave butterflies, then the waves' values in wave order).
template <int NT>
__device__ __forceinline__ double block_max(double v, double* red) {
    v = wave_max(v);
    if constexpr (NT > 64) {
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = red[0];
        for (int q = 1; q < NT / 64; ++q) v = fmax(v, red[q]);
        __syncthreads();
    }
    return v;
}
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if constexpr (NT > 64) {
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = red[0];
        for (int q = 1; q < NT / 64; ++q) v += red[q];
        __syncthreads();
    }
    return v;
}

constexpr int kSteinBatch = 256;   // finished vectors projected out together

// One workgroup of NT threads per cluster (NT = 64 for the clusters of one eigenvalue, which run side by
// side across the chip; more for real clusters, whose cost is the projections).  work: 6 bn-vectors per
// resident workgroup (x, a, b, c, d2, in), stride 6 n.  Wave 0 runs the factorisation and the solves; all
// threads the scalings, norms and projections.  After every solve x is orthogonalised against the
// cluster's finished vectors, kSteinBatch of them at a time: the batch's dots (one wave per vector), then
// x -= sum_p s_p z_p in ascending p: Gram-Schmidt, modified across batches, classical within one (the
// finished vectors are orthonormal to rounding, and the projection is repeated after every solve).
template <int NT>
__global__ __launch_bounds__(NT) void eigh_stein(int n, const double* d, const double* e, const double* w,
                                                 const SteinCluster* clusters, int ncl, const int* items,
                                                 const int* item_k, double* ZT, double* work, int* nfail) {
    constexpr int kMaxIts = 5, kExtra = 2;
    __shared__ double red[16];
    __shared__ double sdot[kSteinBatch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* x = work + (int64_t)blockIdx.x * 6 * n;
    double *a = x + n, *b = a + n, *c = b + n, *d2 = c + n, *in = d2 + n;
    for (int ci = blockIdx.x; ci < ncl; ci += gridDim.x) {
        const SteinCluster cl = clusters[ci];
        const int bn = cl.bn, b0 = cl.b0;
        if (bn == 1) {   // a 1 x 1 block: the unit vector
            if (tid == 0) ZT[b0 + (int64_t)items[cl.first] * n] = 1.0;
            continue;
        }
        const double dtpcrt = sqrt(0.1 / bn);
        double xjm = 0.0;
        for (int t = 0; t < cl.cnt; ++t) {
            const int col = items[cl.first + t];
            double xj = w[col];
            if (t > 0) {   // dstein: eigenvalues closer than 10 eps |lambda| are perturbed apart
                const double pertol = 10.0 * fabs(kEps * xj);
                if (xj - xjm < pertol) xj = xjm + pertol;
            }
            const int kk = item_k[col];
            __syncthreads();
            for (int i = tid; i < bn; i += NT) {
                a[i] = d[b0 + i] - xj;
                const double ei = i < bn - 1 ? e[b0 + i] : 0.0;
                b[i] = ei;
                c[i] = ei;
                x[i] = start_entry(b0, kk, i);
            }
            __syncthreads();
            if (wave == 0) tri_lu_factor(bn, a, b, c, d2, in, lane);
            __syncthreads();
            double tol = 0.0;   // dlagts's default perturbation: eps max(|a|, |b|, |d2|)
            for (int i = tid; i < bn; i += NT) {
                tol = fmax(tol, fabs(a[i]));
                if (i < bn - 1) tol = fmax(tol, fabs(b[i]));
                if (i < bn - 2) tol = fmax(tol, fabs(d2[i]));
            }
            tol = block_max<NT>(tol, red) * kEps;
            if (tol == 0.0) tol = kEps;
            const double alast = fabs(a[bn - 1]);
            int its = 0, nrmchk = 0;
            bool failed = false;
            for (;;) {
                ++its;
                if (its > kMaxIts) { failed = true; break; }
                double xm = 0.0;
                for (int i = tid; i < bn; i += NT) xm = fmax(xm, fabs(x[i]));
                xm = block_max<NT>(xm, red);
                const double scl = (double)bn * cl.onenrm * fmax(kEps, alast) / xm;
                for (int i = tid; i < bn; i += NT) x[i] *= scl;
                __syncthreads();
                if (wave == 0) tri_lu_forward(bn, c, in, x, lane);
                __syncthreads();
                if (wave == 0) tri_lu_backward(bn, a, b, d2, x, tol, lane);
                __syncthreads();
                for (int p0 = 0; p0 < t; p0 += kSteinBatch) {
                    const int np = min(kSteinBatch, t - p0);
                    for (int p = wave; p < np; p += NT / 64) {
                        const double* zp = ZT + b0 + (int64_t)items[cl.first + p0 + p] * n;
                        double s = 0.0;
                        for (int i = lane; i < bn; i += 64) s += x[i] * zp[i];
                        s = wave_sum(s);
                        if (lane == 0) sdot[p] = s;
                    }
                    __syncthreads();
                    for (int i = tid; i < bn; i += NT) {
                        double xi = x[i];
                        for (int p = 0; p < np; ++p) xi -= sdot[p] * ZT[b0 + i + (int64_t)items[cl.first + p0 + p] * n];
                        x[i] = xi;
                    }
                    __syncthreads();
                }
                xm = 0.0;
                for (int i = tid; i < bn; i += NT) xm = fmax(xm, fabs(x[i]));
                xm = block_max<NT>(xm, red);
                if (xm < dtpcrt) continue;
                if (++nrmchk < kExtra + 1) continue;
                break;
            }
            // unit 2-norm, the first largest-modulus entry positive (dstein's normalisation)
            double s2 = 0.0, xm = 0.0;
            for (int i = tid; i < bn; i += NT) {
                s2 += x[i] * x[i];
                xm = fmax(xm, fabs(x[i]));
            }
            s2 = block_sum<NT>(s2, red);
            xm = block_max<NT>(xm, red);
            double firstd = (double)INT_MAX;   // row indices are exact in a double
            for (int i = tid; i < bn; i += NT)
                if (fabs(x[i]) == xm) { firstd = (double)i; break; }
            const int first = (int)-block_max<NT>(-firstd, red);
            __syncthreads();   // x[first] belongs to another thread
            double scl = 1.0 / sqrt(s2);
            if (first < bn && x[first] < 0.0) scl = -scl;
            double* z = ZT + b0 + (int64_t)col * n;
            for (int i = tid; i < bn; i += NT) z[i] = x[i] * scl;
            if (failed && tid == 0) atomicAdd(nfail, 1);
            xjm = xj;
            __syncthreads();   // z is read by the next eigenvalue's projection on other threads' rows
        }
    }
}

// ------------------------------------------------------------------ D Z_T and the final phase
__device__ __forceinline__ double phase_mul(double dd, double z) { return dd * z; }
__device__ __forceinline__ cplx phase_mul(cplx dd, double z) { return cplx{dd.re * z, dd.im * z}; }

template <class S>
__global__ __launch_bounds__(256) void eigh_apply_phase(int n, int64_t m, const S* D, const double* ZT, S* Z) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * m) return;
    Z[idx] = phase_mul(D[idx % n], ZT[idx]);
}

__device__ __forceinline__ double mod_of(double a) { return fabs(a); }
__device__ __forceinline__ double mod_of(cplx a) { return hypot(a.re, a.im); }
__device__ __forceinline__ double fix_phase(double z, double p, double /*pm*/, bool /*at*/) { return p < 0.0 ? -z : z; }
__device__ __forceinline__ cplx fix_phase(cplx z, cplx p, double pm, bool at) {
    if (at) return cplx{pm, 0.0};
    const cplx u{p.re / pm, -p.im / pm};
    return mul(z, u);
}

// one block per column: its largest-modulus entry (the first on ties) made real positive
template <class S>
__global__ __launch_bounds__(256) void eigh_fix_phase(int n, S* Z, int64_t ldz) {
    __shared__ double sv[256];
    __shared__ int si[256];
    S* z = Z + (int64_t)blockIdx.x * ldz;
    double bv = -1.0;
    int bi = INT_MAX;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double v = mod_of(z[i]);
        if (v > bv) { bv = v; bi = i; }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ov = sv[threadIdx.x + s];
            const int oi = si[threadIdx.x + s];
            if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const int k = si[0];
    const double pm = sv[0];
    if (k >= n || !(pm > 0.0)) return;
    const S p = z[k];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) z[i] = fix_phase(z[i], p, pm, i == k);
}

}  // namespace dev

// ============================================================================ host: the plan
namespace {

constexpr double kEpsH = DBL_EPSILON;

// #{eigenvalues of the block [b0, b0 + bn) <= x} by the Sturm recurrence with dstebz's pivmin guard
int64_t sturm_count(const double* d, const double* e, int64_t b0, int64_t bn, double x, double pivmin) {
    int64_t cnt = 0;
    double q = 1.0;
    for (int64_t i = 0; i < bn; ++i) {
        const double ev = i == 0 ? 0.0 : e[b0 + i - 1];
        q = (d[b0 + i] - ev * ev / q) - x;
        if (std::fabs(q) < pivmin) q = -pivmin;
        if (q <= 0.0) ++cnt;
    }
    return cnt;
}

struct TriBlocks {
    std::vector<int64_t> start;     // nblocks + 1
    std::vector<double> onenrm;     // ||T_block||_1
    std::vector<double> pivmin;     // safemin max(1, max e^2)
};

// dstebz's splitting rule
void tridiag_split(int64_t n, const double* d, const double* e, int64_t* block_of, TriBlocks& B) {
    B.start.clear();
    B.onenrm.clear();
    B.pivmin.clear();
    if (n <= 0) {
        B.start.push_back(0);
        return;
    }
    B.start.push_back(0);
    for (int64_t i = 0; i + 1 < n; ++i) {
        const double ae = std::fabs(e[i]);
        // dstebz: e_i^2 <= eps^2 |d_i d_{i+1}| + safemin (an e_i whose square underflows always splits)
        if (ae == 0.0 || ae <= kEpsH * std::sqrt(std::fabs(d[i]) * std::fabs(d[i + 1])) || ae * ae <= DBL_MIN)
            B.start.push_back(i + 1);
    }
    B.start.push_back(n);
    const int64_t nb = (int64_t)B.start.size() - 1;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t b0 = B.start[b], b1 = B.start[b + 1];
        double nrm = 0.0, emax2 = 0.0;
        for (int64_t i = b0; i < b1; ++i) {
            const double el = i > b0 ? std::fabs(e[i - 1]) : 0.0;
            const double er = i + 1 < b1 ? std::fabs(e[i]) : 0.0;
            nrm = std::max(nrm, std::fabs(d[i]) + el + er);
            emax2 = std::max(emax2, er * er);
            if (block_of) block_of[i] = b;
        }
        B.onenrm.push_back(nrm);
        B.pivmin.push_back(DBL_MIN * std::max(1.0, emax2));
    }
}

// The blocks of T = (d, e) and the clusters of the m ascending eigenvalues w: within a block, an
// eigenvalue farther than 1e-3 ||T_block||_1 from the block's previous one starts a new cluster
// (dstein's rule).  owner (optional, m): the block each eigenvalue belongs to, where the caller knows
// it; else it is found from the blocks' Sturm counts (ties between blocks go to the lowest block that
// still has an eigenvalue to give).  Clusters are numbered in the order their first eigenvalue appears.
int tridiag_plan_impl(int64_t n, const double* d, const double* e, int64_t m, const double* w, const int64_t* owner,
                      int64_t* block_of, int64_t* cluster_of, int64_t* owner_out, TriBlocks& B, int64_t* nclusters) {
    tridiag_split(n, d, e, block_of, B);
    const int64_t nb = (int64_t)B.start.size() - 1;
    std::vector<int64_t> own(m, 0);
    if (owner) {
        for (int64_t j = 0; j < m; ++j) {
            if (owner[j] < 0 || owner[j] >= nb) return fail(EIGSOL_E_INVALID, "tridiag_plan: owner out of range");
            own[j] = owner[j];
        }
    } else if (nb > 1 && m > 0) {
        auto tol_of = [&](double x, int64_t b) {
            return 4.0 * kEpsH * std::max(std::fabs(x), B.onenrm[b]) + 2.0 * B.pivmin[b];
        };
        std::vector<int64_t> given(nb);
        for (int64_t b = 0; b < nb; ++b)
            given[b] = sturm_count(d, e, B.start[b], B.start[b + 1] - B.start[b], w[0] - tol_of(w[0], b), B.pivmin[b]);
        for (int64_t j = 0; j < m; ++j) {
            int64_t pick = -1;
            for (int64_t b = 0; b < nb && pick < 0; ++b) {
                const int64_t bn = B.start[b + 1] - B.start[b];
                if (given[b] >= bn) continue;
                if (sturm_count(d, e, B.start[b], bn, w[j] + tol_of(w[j], b), B.pivmin[b]) > given[b]) pick = b;
            }
            if (pick < 0) return fail(EIGSOL_E_INVALID, "tridiag_plan: w holds a value that is no eigenvalue of (d, e)");
            own[j] = pick;
            ++given[pick];
        }
    }
    std::vector<double> lastw(nb, 0.0);
    std::vector<int64_t> cur(nb, -1);
    int64_t ncl = 0;
    for (int64_t j = 0; j < m; ++j) {
        const int64_t b = own[j];
        if (cur[b] < 0 || std::fabs(w[j] - lastw[b]) > 1e-3 * B.onenrm[b]) cur[b] = ncl++;
        lastw[b] = w[j];
        if (cluster_of) cluster_of[j] = cur[b];
        if (owner_out) owner_out[j] = b;
    }
    if (nclusters) *nclusters = ncl;
    return EIGSOL_OK;
}

template <class S> struct EighOps;
template <> struct EighOps<double> {
    static int reduce(hipStream_t st, double* A, int64_t n, double* V, double* T) { return hessenberg_blocked_vt_f64(st, A, n, V, T); }
    static int back(hipStream_t st, int64_t n, int64_t m, const double* V, const double* T, double* Z) {
        return hess_backtransform_f64(st, n, m, V, T, Z, n);
    }
    static int nb() { return hess_panel_width_f64(); }
    static double one() { return 1.0; }
    static double mulp(double a, double b) { return a * b; }
};
template <> struct EighOps<cplx> {
    static int reduce(hipStream_t st, cplx* A, int64_t n, cplx* V, cplx* T) { return hessenberg_blocked_vt_c128(st, A, n, V, T); }
    static int back(hipStream_t st, int64_t n, int64_t m, const cplx* V, const cplx* T, cplx* Z) {
        return hess_backtransform_c128(st, n, m, V, T, Z, n);
    }
    static int nb() { return hess_panel_width_c128(); }
    static cplx one() { return cplx{1.0, 0.0}; }
    static cplx mulp(cplx a, cplx b) {
        cplx r{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
        const double h = std::hypot(r.re, r.im);   // keep the accumulated phase on the unit circle
        if (h > 0.0) { r.re /= h; r.im /= h; }
        return r;
    }
};

struct EigItem {
    double lam;
    int64_t block, k;
};

// The solver on a matrix already on the device (dA: n x n, its lower triangle read; freed once reduced).
// w_out (host) receives the m selected eigenvalues; with `vectors` dZ receives Z (n x m, on the device),
// which is also copied to Z_host where that is given.  fix_phase: apply the phase convention to Z.
template <class S>
int eigh_core(eigsol_ctx* ctx, int64_t n, DevBuf& dA, int select, int64_t il, int64_t iu, double vl, double vu,
              int method, double* w_out, bool vectors, bool fix_phase, void* Z_host, DevBuf& dZ, int64_t* m_out,
              int64_t* not_converged) {
    using Ops = EighOps<S>;
    // divide and conquer forms vectors with its values: a values-only call stays the bisection path
    const bool dc = method == EIGSOL_EIGH_METHOD_DC && vectors;
    hipStream_t st = ctx->stream;
    const int NB = Ops::nb();
    const int64_t npan = n >= 3 ? (n - 2 + NB - 1) / NB : 0;
    StageClock clock;
    EIGSOL_TRY(clock.start(4));
    DevBuf dV, dT, dd, de, dph;
    EIGSOL_TRY(dd.alloc((size_t)n * sizeof(double)));
    // e (n entries), then the scaling's scratch: kAbsmaxBlocks partial maxima and the exponent
    EIGSOL_TRY(de.alloc((size_t)(n + dev::kAbsmaxBlocks + 1) * sizeof(double)));
    double* const dmax = de.as<double>() + n;
    int* const dkexp = reinterpret_cast<int*>(dmax + dev::kAbsmaxBlocks);
    EIGSOL_TRY(dph.alloc((size_t)n * sizeof(S)));
    if (vectors && npan) {
        EIGSOL_TRY(dV.alloc((size_t)npan * n * NB * sizeof(S)));
        EIGSOL_TRY(dT.alloc((size_t)npan * NB * NB * sizeof(S)));
    }
    EIGSOL_TRY(clock.mark(0, st));
    const unsigned gnn = (unsigned)(((int64_t)n * n + 255) / 256);
    const unsigned gmax = std::min<unsigned>(gnn, dev::kAbsmaxBlocks);
    hipLaunchKernelGGL(dev::eigh_absmax<S>, dim3(gmax), dim3(256), 0, st, dA.as<S>(), (int)n, dmax);
    hipLaunchKernelGGL(dev::eigh_rescale<S>, dim3(std::min<unsigned>(gnn, dev::kRescaleBlocks)), dim3(256), 0, st, dA.as<S>(),
                       (int)n, dmax, (int)gmax, dkexp);
    hipLaunchKernelGGL(dev::eigh_symmetrise<S>, dim3(gnn), dim3(256), 0, st, dA.as<S>(), (int)n);
    EIGSOL_TRY(Ops::reduce(st, dA.as<S>(), n, dV.as<S>(), dT.as<S>()));
    hipLaunchKernelGGL(dev::eigh_extract<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dA.as<S>(), (int)n,
                       dd.as<double>(), de.as<double>(), dph.as<S>());
    EIGSOL_HIP(hipGetLastError());
    std::vector<double> d(n), e(std::max<int64_t>(n, 1), 0.0);
    std::vector<S> ph(std::max<int64_t>(n, 1));
    EIGSOL_HIP(hipMemcpyAsync(d.data(), dd.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n > 1) {
        EIGSOL_HIP(hipMemcpyAsync(e.data(), de.p, (size_t)(n - 1) * sizeof(double), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(ph.data(), dph.p, (size_t)(n - 1) * sizeof(S), hipMemcpyDeviceToHost, st));
    }
    int kexp = 0;   // the matrix reduced is 2^kexp A
    EIGSOL_HIP(hipMemcpyAsync(&kexp, dkexp, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(1, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(d[i]) || !std::isfinite(e[i]))
            return fail(EIGSOL_E_SOLVER, "eigh: the lower triangle holds a non-finite entry");
    dA.release();   // the reduced matrix is not read again

    // ---- d. split; e. bisection of every block of order >= 2
    TriBlocks B;
    tridiag_split(n, d.data(), e.data(), nullptr, B);
    const int64_t nblocks = (int64_t)B.start.size() - 1;
    std::vector<dev::BisectWave> waves;
    std::vector<double> lam(n);
    DevBuf dQdc;        // dc: the eigenvectors of T, column i belongs to lam[i]
    int64_t ncap = 0;   // dc: leaf eigenvalues and secular roots that hit their iteration cap
    if (dc) {           // ---- e, f. by divide and conquer (eigh_dc.hip); slot 1 of the stage times stays 0
        EIGSOL_TRY(clock.mark(2, st));
        EIGSOL_TRY(eigh_dc_tridiag(ctx, n, d.data(), e.data(), B.start, dQdc, lam.data(), &ncap));
    }
    for (int64_t b = 0; b < nblocks && !dc; ++b) {
        const int64_t b0 = B.start[b], bn = B.start[b + 1] - b0;
        if (bn == 1) {
            lam[b0] = d[b0];
            continue;
        }
        double gl = d[b0], gu = d[b0];
        for (int64_t i = b0; i < b0 + bn; ++i) {
            const double r = (i > b0 ? std::fabs(e[i - 1]) : 0.0) + (i + 1 < b0 + bn ? std::fabs(e[i]) : 0.0);
            gl = std::min(gl, d[i] - r);
            gu = std::max(gu, d[i] + r);
        }
        const double tnorm = std::max(std::fabs(gl), std::fabs(gu));
        gl = gl - 2.1 * tnorm * kEpsH * (double)bn - 2.1 * B.pivmin[b];
        gu = gu + 2.1 * tnorm * kEpsH * (double)bn + 2.1 * B.pivmin[b];
        for (int64_t k0 = 0; k0 < bn; k0 += 64)
            waves.push_back(dev::BisectWave{(int)b0, (int)bn, (int)k0, (int)std::min<int64_t>(64, bn - k0), gl, gu, B.pivmin[b]});
    }
    DevBuf dwv, dlam;
    if (!waves.empty()) {
        EIGSOL_TRY(dwv.alloc(waves.size() * sizeof(dev::BisectWave)));
        EIGSOL_TRY(dlam.alloc((size_t)n * sizeof(double)));
        EIGSOL_HIP(hipMemcpyAsync(dwv.p, waves.data(), waves.size() * sizeof(dev::BisectWave), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dlam.p, lam.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(dev::eigh_bisect, dim3((unsigned)waves.size()), dim3(64), 0, st, dd.as<double>(), de.as<double>(),
                           dwv.as<dev::BisectWave>(), dlam.as<double>());
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_HIP(hipMemcpyAsync(lam.data(), dlam.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (!dc) EIGSOL_TRY(clock.mark(2, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    // ascending; equal values in block order (a fixed order, whatever the selection)
    std::vector<EigItem> all(n);
    for (int64_t b = 0; b < nblocks; ++b)
        for (int64_t i = B.start[b]; i < B.start[b + 1]; ++i) all[i] = EigItem{lam[i], b, i - B.start[b]};
    std::sort(all.begin(), all.end(), [](const EigItem& x, const EigItem& y) {
        if (x.lam != y.lam) return x.lam < y.lam;
        if (x.block != y.block) return x.block < y.block;
        return x.k < y.k;
    });
    int64_t s0 = 0, s1 = n;   // [s0, s1) of the sorted list
    if (select == EIGSOL_EIGH_INDEX) {
        s0 = il;
        s1 = iu + 1;
    } else if (select == EIGSOL_EIGH_VALUE) {
        s0 = 0;
        while (s0 < n && !(std::ldexp(all[s0].lam, -kexp) > vl)) ++s0;   // vl, vu are on the caller's scale
        s1 = s0;
        while (s1 < n && std::ldexp(all[s1].lam, -kexp) <= vu) ++s1;
    }
    const int64_t m = s1 - s0;
    *m_out = m;
    std::vector<double> ws(m);   // the selected eigenvalues of the scaled matrix, which the vectors are computed from
    for (int64_t j = 0; j < m; ++j) {
        ws[j] = all[s0 + j].lam;
        w_out[j] = std::ldexp(ws[j], -kexp);   // exact; kexp = 0 leaves the bits
    }
    if (not_converged) *not_converged = 0;
    double* const ms = ctx->eigh_ms;
    if (!vectors || m == 0) {
        if (dc) {   // an empty value range: the whole tridiagonal stage ran
            EIGSOL_TRY(clock.mark(3, st));
            EIGSOL_HIP(hipStreamSynchronize(st));
        }
        clock.read(ms, 4);   // the stages marked so far
        if (dc) {
            ms[1] = 0.0;
            ctx->eigh_dc_ms[0] = ms[0];
            ctx->eigh_dc_ms[5] = 0.0;
        }
        return EIGSOL_OK;
    }

    // ---- f. Z_T (n x m): the selected columns of divide and conquer's vector matrix, or inverse iteration
    DevBuf dZT, dD;
    DevBuf dw, dcl, dit, dik, dwork, dfail;   // inverse iteration's; with the host arrays its uploads read,
    std::vector<dev::SteinCluster> sorted;    // they live until the stream is waited for
    std::vector<int> items, item_k;
    EIGSOL_TRY(dZT.alloc((size_t)n * m * sizeof(double)));
    EIGSOL_TRY(dD.alloc((size_t)n * sizeof(S)));
    EIGSOL_TRY(dZ.alloc((size_t)n * m * sizeof(S)));
    std::vector<S> D(n);
    D[0] = Ops::one();
    for (int64_t i = 0; i + 1 < n; ++i) D[i + 1] = Ops::mulp(D[i], ph[i]);
    int nfail = 0;
    if (dc) {   // the workspace goes before the back-transformation
        std::vector<int> cols(m);
        for (int64_t j = 0; j < m; ++j) cols[j] = (int)(B.start[all[s0 + j].block] + all[s0 + j].k);
        EIGSOL_TRY(eigh_dc_take_columns(st, n, m, dQdc.as<double>(), cols, dZT.as<double>()));
        dQdc.release();
        EIGSOL_HIP(hipMemcpyAsync(dD.p, D.data(), (size_t)n * sizeof(S), hipMemcpyHostToDevice, st));
    } else {    // clusters (the same plan eigsol_tridiag_plan returns) and inverse iteration
        std::vector<int64_t> owner(m), cluster_of(m);
        for (int64_t j = 0; j < m; ++j) owner[j] = all[s0 + j].block;
        int64_t ncl = 0;
        EIGSOL_TRY(tridiag_plan_impl(n, d.data(), e.data(), m, ws.data(), owner.data(), nullptr, cluster_of.data(), nullptr, B, &ncl));
        std::vector<dev::SteinCluster> cls(ncl, dev::SteinCluster{0, 0, 0, 0, 0.0});
        for (int64_t j = 0; j < m; ++j) {
            dev::SteinCluster& c = cls[cluster_of[j]];
            if (c.cnt == 0) {
                c.b0 = (int)B.start[owner[j]];
                c.bn = (int)(B.start[owner[j] + 1] - B.start[owner[j]]);
                c.onenrm = B.onenrm[owner[j]];
            }
            ++c.cnt;
        }
        // clusters of one eigenvalue (one wave each) first, then the real clusters (one large workgroup each)
        std::vector<int64_t> order;
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t c = 0; c < ncl; ++c)
                if ((cls[c].cnt == 1) == (pass == 0)) order.push_back(c);
        sorted.resize(ncl);
        std::vector<int64_t> place(ncl);
        int run = 0;
        int64_t nsingle = 0;
        for (int64_t q = 0; q < ncl; ++q) {
            sorted[q] = cls[order[q]];
            sorted[q].first = run;
            run += sorted[q].cnt;
            place[order[q]] = q;
            if (sorted[q].cnt == 1) ++nsingle;
        }
        items.assign(m, 0);
        item_k.assign(m, 0);
        std::vector<int> fill(ncl, 0);
        for (int64_t j = 0; j < m; ++j) {
            const int64_t q = place[cluster_of[j]];
            items[sorted[q].first + fill[q]++] = (int)j;   // ascending within the cluster
            item_k[j] = (int)all[s0 + j].k;
        }
        constexpr int kClusterThreads = 1024;
        const int slots1 = (int)std::min<int64_t>(nsingle, 2048), slots2 = (int)std::min<int64_t>(ncl - nsingle, 512);
        EIGSOL_TRY(dw.alloc((size_t)m * sizeof(double)));
        EIGSOL_TRY(dcl.alloc((size_t)ncl * sizeof(dev::SteinCluster)));
        EIGSOL_TRY(dit.alloc((size_t)m * sizeof(int)));
        EIGSOL_TRY(dik.alloc((size_t)m * sizeof(int)));
        EIGSOL_TRY(dwork.alloc((size_t)(slots1 + slots2) * 6 * n * sizeof(double)));
        EIGSOL_TRY(dfail.alloc(64));
        EIGSOL_HIP(hipMemcpyAsync(dw.p, ws.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dcl.p, sorted.data(), (size_t)ncl * sizeof(dev::SteinCluster), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dit.p, items.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dik.p, item_k.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemsetAsync(dZT.p, 0, (size_t)n * m * sizeof(double), st));
        EIGSOL_HIP(hipMemsetAsync(dfail.p, 0, 64, st));
        EIGSOL_HIP(hipMemcpyAsync(dD.p, D.data(), (size_t)n * sizeof(S), hipMemcpyHostToDevice, st));
        if (slots2)
            hipLaunchKernelGGL(dev::eigh_stein<kClusterThreads>, dim3(slots2), dim3(kClusterThreads), 0, st, (int)n,
                               dd.as<double>(), de.as<double>(), dw.as<double>(), dcl.as<dev::SteinCluster>() + nsingle,
                               (int)(ncl - nsingle), dit.as<int>(), dik.as<int>(), dZT.as<double>(),
                               dwork.as<double>() + (size_t)slots1 * 6 * n, dfail.as<int>());
        if (slots1)
            hipLaunchKernelGGL(dev::eigh_stein<64>, dim3(slots1), dim3(64), 0, st, (int)n, dd.as<double>(), de.as<double>(),
                               dw.as<double>(), dcl.as<dev::SteinCluster>(), (int)nsingle, dit.as<int>(), dik.as<int>(),
                               dZT.as<double>(), dwork.as<double>(), dfail.as<int>());
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_HIP(hipMemcpyAsync(&nfail, dfail.p, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    EIGSOL_TRY(clock.mark(3, st));

    // ---- g. Z = Q (D Z_T), then the phase convention
    const unsigned gnm = (unsigned)(((int64_t)n * m + 255) / 256);
    hipLaunchKernelGGL(dev::eigh_apply_phase<S>, dim3(gnm), dim3(256), 0, st, (int)n, m, dD.as<S>(), dZT.as<double>(), dZ.as<S>());
    if (npan) EIGSOL_TRY(Ops::back(st, n, m, dV.as<S>(), dT.as<S>(), dZ.as<S>()));
    if (fix_phase) hipLaunchKernelGGL(dev::eigh_fix_phase<S>, dim3((unsigned)m), dim3(256), 0, st, (int)n, dZ.as<S>(), n);
    EIGSOL_HIP(hipGetLastError());
    if (Z_host) EIGSOL_HIP(hipMemcpyAsync(Z_host, dZ.p, (size_t)n * m * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(4, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (not_converged) *not_converged = dc ? ncap : nfail;
    clock.read(ms, 4);
    if (dc) {
        ms[1] = 0.0;
        ctx->eigh_dc_ms[0] = ms[0];
        ctx->eigh_dc_ms[5] = ms[3];
    }
    return EIGSOL_OK;
}

template <class S>
int eigh_host(eigsol_ctx* ctx, int64_t n, const void* A_host, int select, int64_t il, int64_t iu, double vl, double vu,
              int method, double* w_out, void* Z_out, int64_t* m_out, int64_t* not_converged) {
    DevBuf dA, dZ;
    EIGSOL_TRY(dA.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_HIP(hipMemcpyAsync(dA.p, A_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, ctx->stream));
    return eigh_core<S>(ctx, n, dA, select, il, iu, vl, vu, method, w_out, Z_out != nullptr, true, Z_out, dZ, m_out, not_converged);
}

}  // namespace

int eigh_device_m(eigsol_ctx* ctx, int dtype, int64_t n, DevBuf& dA, int select, int64_t il, int64_t iu, double vl,
                  double vu, int method, double* w_out, bool vectors, DevBuf& dZ, int64_t* m_out, int64_t* not_converged) {
    return dtype == EIGSOL_C128
               ? eigh_core<cplx>(ctx, n, dA, select, il, iu, vl, vu, method, w_out, vectors, false, nullptr, dZ, m_out, not_converged)
               : eigh_core<double>(ctx, n, dA, select, il, iu, vl, vu, method, w_out, vectors, false, nullptr, dZ, m_out, not_converged);
}

int eigh_device(eigsol_ctx* ctx, int dtype, int64_t n, DevBuf& dA, int select, int64_t il, int64_t iu, double vl,
                double vu, double* w_out, bool vectors, DevBuf& dZ, int64_t* m_out, int64_t* not_converged) {
    return eigh_device_m(ctx, dtype, n, dA, select, il, iu, vl, vu, EIGSOL_EIGH_METHOD_STEIN, w_out, vectors, dZ, m_out,
                         not_converged);
}

int eigh_fix_phase_device(hipStream_t st, int dtype, int64_t n, int64_t m, void* Z) {
    if (m <= 0) return EIGSOL_OK;
    if (dtype == EIGSOL_C128)
        hipLaunchKernelGGL(dev::eigh_fix_phase<cplx>, dim3((unsigned)m), dim3(256), 0, st, (int)n, static_cast<cplx*>(Z), n);
    else
        hipLaunchKernelGGL(dev::eigh_fix_phase<double>, dim3((unsigned)m), dim3(256), 0, st, (int)n, static_cast<double*>(Z), n);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

int eigh_parse_selection(const char* who, int64_t n, const eigsol_eigh_options* opts, int* select, int64_t* il,
                         int64_t* iu, double* vl, double* vu) {
    *select = opts ? opts->select : EIGSOL_EIGH_ALL;
    *il = 0;
    *iu = n - 1;
    *vl = *vu = 0.0;
    if (*select == EIGSOL_EIGH_INDEX) {
        *il = opts->il;
        *iu = opts->iu;
        if (*il > *iu || *il < 0 || *iu >= n) return fail(EIGSOL_E_INVALID, std::string(who) + ": index range outside 0 <= il <= iu < n");
    } else if (*select == EIGSOL_EIGH_VALUE) {
        *vl = opts->vl;
        *vu = opts->vu;
        if (std::isnan(*vl) || std::isnan(*vu) || !(*vl < *vu)) return fail(EIGSOL_E_INVALID, std::string(who) + ": value range needs vl < vu");
    } else if (*select != EIGSOL_EIGH_ALL) {
        return fail(EIGSOL_E_INVALID, std::string(who) + ": unknown selection");
    }
    return EIGSOL_OK;
}

}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_tridiag_plan(int64_t n, const double* d, const double* e, int64_t m, const double* w, int64_t* block_of,
                        int64_t* cluster_of, int64_t* nblocks, int64_t* nclusters) {
    if (n < 0 || m < 0 || m > n || !nblocks || !nclusters || (n > 0 && (!d || !block_of)) || (n > 1 && !e) ||
        (m > 0 && (!w || !cluster_of)))
        return fail(EIGSOL_E_INVALID, "eigsol_tridiag_plan: bad arguments");
    for (int64_t j = 1; j < m; ++j)
        if (!(w[j - 1] <= w[j])) return fail(EIGSOL_E_INVALID, "eigsol_tridiag_plan: w must be ascending");
    TriBlocks B;
    int64_t ncl = 0;
    EIGSOL_TRY(tridiag_plan_impl(n, d, e, m, w, nullptr, block_of, cluster_of, nullptr, B, &ncl));
    *nblocks = n > 0 ? (int64_t)B.start.size() - 1 : 0;
    *nclusters = ncl;
    return EIGSOL_OK;
}

int eigsol_eigh_dense_m(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_eigh_options* opts,
                        int32_t method, double* w, void* Z, int64_t* m_out, int64_t* not_converged) {
    if (method != EIGSOL_EIGH_METHOD_STEIN && method != EIGSOL_EIGH_METHOD_DC)
        return fail(EIGSOL_E_INVALID, "eigsol_eigh_dense: unknown method");
    if (n < 0) return fail(EIGSOL_E_INVALID, "eigsol_eigh_dense: negative order");
    if (n == 0) {
        if (m_out) *m_out = 0;
        if (not_converged) *not_converged = 0;
        return EIGSOL_OK;
    }
    if (!ctx || !A_colmajor || !w || !m_out) return fail(EIGSOL_E_INVALID, "eigsol_eigh_dense: null pointer");
    int select;
    int64_t il, iu;
    double vl, vu;
    EIGSOL_TRY(eigh_parse_selection("eigsol_eigh_dense", n, opts, &select, &il, &iu, &vl, &vu));
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_eigh_dense: double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, "eigsol_eigh_dense: unknown dtype");
    if (n > (dtype == EIGSOL_C128 ? hess_max_order_c128() : hess_max_order_f64()))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_eigh_dense: n above the order the blocked Hessenberg reduction accepts");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return dtype == EIGSOL_C128
               ? eigh_host<cplx>(ctx, n, A_colmajor, select, il, iu, vl, vu, method, w, Z, m_out, not_converged)
               : eigh_host<double>(ctx, n, A_colmajor, select, il, iu, vl, vu, method, w, Z, m_out, not_converged);
}

int eigsol_eigh_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_eigh_options* opts,
                      double* w, void* Z, int64_t* m_out, int64_t* not_converged) {
    return eigsol_eigh_dense_m(ctx, dtype, n, A_colmajor, opts, EIGSOL_EIGH_METHOD_STEIN, w, Z, m_out, not_converged);
}

int eigsol_eigh_dc_stage_times(eigsol_ctx* ctx, double* ms6) {
    if (!ctx || !ms6) return fail(EIGSOL_E_INVALID, "eigsol_eigh_dc_stage_times: null pointer");
    for (int q = 0; q < 6; ++q) ms6[q] = ctx->eigh_dc_ms[q];
    return EIGSOL_OK;
}

int eigsol_eigh_stage_times(eigsol_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return fail(EIGSOL_E_INVALID, "eigsol_eigh_stage_times: null pointer");
    for (int q = 0; q < 4; ++q) ms4[q] = ctx->eigh_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
