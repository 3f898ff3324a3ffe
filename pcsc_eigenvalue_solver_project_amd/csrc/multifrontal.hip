// Nested-dissection multifrontal LU of M = A - sigma I on gfx950, for general sparse patterns whose
// LU has real fill (a 2-D or 3-D mesh under any numbering).
//
// Replaces the SparseLU branch of solve_shifted<S> (src/matrix/solve_shifted.hpp:85-117: M = A,
// M(i, i) -= sigma with coeffRef inserting a missing diagonal :96-102, analyzePattern + factorize
// :104-106, solve :112-115).  SparseLU orders columns with COLAMD and factors supernodes on one
// core; here the order is a nested dissection of the pattern of M + M^T and the factorization is
// multifrontal, so that the work is dense blocks on the matrix cores and independent fronts run
// side by side:
//   * ordering (host): recursive bisection of the graph by breadth-first level structures from a
//     pseudo-peripheral vertex; the median level, thinned to the vertices that touch the next
//     level, is the separator; pieces of at most EIGSOL_MF_LEAF (64) vertices are leaves;
//     disconnected pieces are split into components and the small ones packed together.  The
//     tree is numbered in postorder, so every supernode (a leaf or a separator) owns a contiguous
//     range of columns and its descendants come before it;
//   * symbolic (host): struct(s) = the indices past s's columns that s's rows reach in M + M^T or
//     through a child's struct; the front of s is the dense (ns + ms)^2 matrix on the index list
//     [s's columns, struct(s)], column-major, resident in HBM for the factor's lifetime;
//   * numeric (device, by tree height, all fronts of a height in the same launches): M's entries
//     scattered into their fronts once; per height the children's Schur blocks extend-added into
//     their parents (one launch per child rank, so the sum order is fixed); then panels of NB
//     pivots: one workgroup per front factors its panel with partial pivoting restricted to the
//     front's own pivot rows (no delayed pivots; a zero pivot fails the factor), swaps whole rows
//     (LAPACK getrf style) and solves U12 = L11^-1 A12; one batched launch runs every front's
//     trailing update A22 -= L21 U12 on the fp64 matrix cores (rankk_tile, 64 x 64 tiles, all
//     fronts of the height in one grid).  The trailing block left after the last panel is the
//     Schur complement the parent receives;
//   * solve: gather b into the new numbering; forward by height (one workgroup per front: the
//     children's contribution vectors extend-added in a fixed order, the pivot permutation, the
//     unit-lower L11 solve by 64-row blocks - the block's triangle on one wave by lane broadcasts,
//     the rows below as a GEMV by the workgroup - and the front's own contribution L21 y); then
//     backward from the root (x of struct(s) gathered from the ancestors, y - U12 x, the U11
//     solve by blocks from the bottom); scatter back.  Every sum has a fixed order: the solve is
//     deterministic.
// The pivoting is restricted to each front, so the factor is the exact LU of a row-permuted M
// only when no pivot is tiny; gmres.hip therefore treats it like the no-pivot exact LU: the solve
// is checked by its true residual and refined by GMRES cycles on the same factor when it misses.
// This file is the device half: the kernels, the factor's device state and the solve's launches.
// The host half (ordering, symbolic structure, launch and solve tables) is multifrontal_plan.cpp,
// plain C++ behind multifrontal_plan.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kernels_common.hpp"
#include "mfma_rankk.hpp"
#include "multifrontal_plan.hpp"

namespace eigsol {

static_assert(kMfPanelF64 == dev::RankKMax<double>::value && kMfPanelC128 == dev::RankKMax<cplx>::value,
              "multifrontal_plan.hpp: the plan's panel widths are the rank-k tile's");

namespace dev {

__device__ __forceinline__ double mf_rl(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ cplx mf_rl(cplx v, int src) { return cplx{mf_rl(v.re, src), mf_rl(v.im, src)}; }
// write-through stores / agent-scope loads of values handed between workgroups of one launch
__device__ __forceinline__ void mf_st(double* p, double v) { st_agent(p, v); }
__device__ __forceinline__ void mf_st(cplx* p, cplx v) {
    st_agent(&p->re, v.re);
    st_agent(&p->im, v.im);
}
__device__ __forceinline__ double mf_ld(const double* p) { return ld_agent(p); }
__device__ __forceinline__ cplx mf_ld(const cplx* p) { return cplx{ld_agent(&p->re), ld_agent(&p->im)}; }

// value flags of the row-block solve (EIGSOL_MF_VALFLAG): an unsolved pivot value holds this NaN in
// every 8-byte word, a solved one never does (a NaN result is stored as the default quiet NaN), so a
// waiting block polls the values themselves instead of a flag and then the values
constexpr int kMfUnroll = 8;   // loads in flight per thread in the small fronts' inverse-form products
constexpr unsigned long long kMfSent = 0x7FF4DEAD7FF4DEADull;
__device__ __forceinline__ bool mf_unready(double v) { return (unsigned long long)__double_as_longlong(v) == kMfSent; }
__device__ __forceinline__ bool mf_unready(cplx v) { return mf_unready(v.re) || mf_unready(v.im); }
__device__ __forceinline__ double mf_sent(double) { return __longlong_as_double((long long)kMfSent); }
__device__ __forceinline__ cplx mf_sent(cplx) { return cplx{mf_sent(0.0), mf_sent(0.0)}; }
__device__ __forceinline__ double mf_clean(double v) { return v != v ? __longlong_as_double(0x7FF8000000000000ll) : v; }
__device__ __forceinline__ cplx mf_clean(cplx v) { return cplx{mf_clean(v.re), mf_clean(v.im)}; }
template <class S>
__device__ __forceinline__ S mf_poll(const S* p, int32_t* err, int bo) {
    S v = mf_ld(p);
    int spins = 0;
    while (mf_unready(v)) {
        if (!(bo & 1)) __builtin_amdgcn_s_sleep(1);
        else if (spins < 4) __builtin_amdgcn_s_sleep(2);
        else __builtin_amdgcn_s_sleep(8);
        v = mf_ld(p);
        if (++spins > (1 << 22)) {
            atomicOr(err, 4);
            break;
        }
    }
    return v;
}

// M's entries into their fronts: F[dst[e]] = v[e] (every destination distinct)
template <class S>
__global__ __launch_bounds__(256) void mf_scatter_kernel(const int64_t* dst, const S* v, int64_t nnz, S* F) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nnz) F[dst[e]] = v[e];
}

// extend-add of one child's Schur block into its parent: tab = (child, first column) pairs, 64
// columns per workgroup; children of one parent are in different launches (fixed order)
template <class S>
__global__ __launch_bounds__(256) void mf_extend_kernel(const MfFront* fr, const int32_t* tab, const int32_t* cmap,
                                                        S* F) {
    const int32_t c = tab[2 * blockIdx.x], col0 = tab[2 * blockIdx.x + 1];
    const MfFront fc = fr[c];
    const MfFront fp = fr[fc.parent];
    const int32_t* map = cmap + fc.sof;
    const S* src = F + fc.off + (int64_t)fc.ns * (fc.d + 1);
    S* dst = F + fp.off;
    const int cend = min(fc.ms, col0 + 64);
    for (int cc = col0; cc < cend; ++cc) {
        const int64_t pc = (int64_t)map[cc] * fp.d;
        const S* sc = src + (int64_t)cc * fc.d;
        for (int r = threadIdx.x; r < fc.ms; r += 256) {
            const int64_t o = pc + map[r];
            dst[o] = add(dst[o], sc[r]);
        }
    }
}

// a / b for a pivot b whose squared modulus underflows (exact power-of-two scaling of b)
__device__ inline double sdiv_tiny(double a, double b) { return a / b; }
__device__ inline cplx sdiv_tiny(cplx a, cplx b) {
    const cplx q = cdiv(a, cplx{ldexp(b.re, 600), ldexp(b.im, 600)});
    return cplx{ldexp(q.re, 600), ldexp(q.im, 600)};
}

// Panel q of every front in list[0 .. gridDim.x): pivots k0 .. k0 + kb - 1 (k0 = q NB), each the
// first row of largest modulus among the front's remaining pivot rows [k, ns); the whole row
// swapped (all d columns), the column below the diagonal scaled, the panel's other columns
// rank-1 updated; then U12 = L11^-1 A12 on the columns right of the panel (one column per thread).
// tau > 0 (static pivoting, the retry after a zero pivot): a pivot column whose remaining front
// rows are all exactly zero gets the pivot tau on its diagonal (counted in *nstat) instead of
// failing - a perturbation of M that the checked solve's GMRES refinement then removes.
template <class S, int NB>
__global__ __launch_bounds__(256) void mf_panel_kernel(const MfFront* fr, const int32_t* list, int q, S* F,
                                                       int32_t* piv, int32_t* zpiv, double tau, int32_t* nstat) {
    __shared__ double sv[4];
    __shared__ int si[4];
    __shared__ int s_p, s_fix;
    __shared__ S l11[NB * NB];
    const MfFront f = fr[list[blockIdx.x]];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int d = f.d, ns = f.ns;
    const int k0 = q * NB, kb = min(NB, ns - k0), c1 = k0 + kb;
    S* A = F + f.off;
    for (int k = k0; k < c1; ++k) {
        double best = -1.0;
        int bi = k;
        for (int i = k + tid; i < ns; i += 256) {
            const double s = mod_abs(A[i + (int64_t)k * d]);   // no underflow below |a| ~ 1e-162
            if (s > best) { best = s; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { sv[wv] = best; si[wv] = bi; }
        __syncthreads();
        if (tid == 0) {
            double b = sv[0];
            int p = si[0];
            for (int w = 1; w < 4; ++w)
                if (sv[w] > b || (sv[w] == b && si[w] < p)) { b = sv[w]; p = si[w]; }
            s_p = p;
            piv[f.c0 + k] = p;
            s_fix = 0;
            if (!(b > 0.0)) {
                if (tau > 0.0) {
                    s_fix = 1;
                    atomicAdd(nstat, 1);
                } else {
                    atomicOr(zpiv, 1);
                }
            }
        }
        __syncthreads();
        const int p = s_p;
        if (s_fix) {   // the whole column is zero in the front's rows: p == k, no interchange
            if (tid == 0) set_re_im(A[k + (int64_t)k * d], tau, 0.0);
            __syncthreads();
        }
        if (p != k)
            for (int j = tid; j < d; j += 256) {
                const S t = A[k + (int64_t)j * d];
                A[k + (int64_t)j * d] = A[p + (int64_t)j * d];
                A[p + (int64_t)j * d] = t;
            }
        __syncthreads();
        const S dk = A[k + (int64_t)k * d];
        if (sq_abs(dk) >= 1e-280) {
            for (int i = k + 1 + tid; i < d; i += 256) A[i + (int64_t)k * d] = sdiv(A[i + (int64_t)k * d], dk);
        } else if (mod_abs(dk) > 0.0) {
            // |pivot| below ~1e-140: its squared modulus (the textbook complex quotient's
            // denominator) would underflow; divide by the pivot scaled by 2^600, then rescale
            for (int i = k + 1 + tid; i < d; i += 256) A[i + (int64_t)k * d] = sdiv_tiny(A[i + (int64_t)k * d], dk);
        }
        __syncthreads();
        const int m = d - k - 1, w = c1 - k - 1;
        for (int e = tid; e < m * w; e += 256) {
            const int i = k + 1 + e % m, j = k + 1 + e / m;
            A[i + (int64_t)j * d] = sub(A[i + (int64_t)j * d], mul(A[i + (int64_t)k * d], A[k + (int64_t)j * d]));
        }
        __syncthreads();
    }
    for (int e = tid; e < kb * kb; e += 256) {
        const int i = e % kb, j = e / kb;
        l11[i + j * NB] = A[(k0 + i) + (int64_t)(k0 + j) * d];
    }
    __syncthreads();
    for (int c = c1 + tid; c < d; c += 256) {
        S* col = A + (int64_t)c * d + k0;
        S x[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) x[i] = i < kb ? col[i] : s_zero<S>();
#pragma unroll
        for (int j = 0; j < NB - 1; ++j) {
            if (j < kb) {
#pragma unroll
                for (int i = j + 1; i < NB; ++i) x[i] = sub(x[i], mul(l11[i + j * NB], x[j]));
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (i < kb) col[i] = x[i];
    }
}

// trailing update of panel q, every front of the launch: tab = (front, tile row, tile column)
template <class S, int NB>
__global__ __launch_bounds__(256) void mf_gemm_kernel(const MfFront* fr, const int32_t* tab, int q, S* F) {
    const int32_t s = tab[3 * blockIdx.x], tr = tab[3 * blockIdx.x + 1], tc = tab[3 * blockIdx.x + 2];
    const MfFront f = fr[s];
    const int d = f.d, k0 = q * NB, kb = min(NB, f.ns - k0), c1 = k0 + kb, m = d - c1;
    S* A = F + f.off;
    rankk_tile<S, true>(tr, tc, m, m, kb, -1.0, A + c1 + (int64_t)k0 * d, d, A + k0 + (int64_t)c1 * d, d,
                        A + c1 + (int64_t)c1 * d, d);
}

// ---------------------------------------------------------------- solve
// w = b in the new numbering
template <class S>
__global__ __launch_bounds__(256) void mf_gather_kernel(const int32_t* perm, const S* b, S* w, int64_t n,
                                                        const uint8_t* bigm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i] = (bigm && bigm[i]) ? mf_sent(s_zero<S>()) : b[perm[i]];   // bigm: large fronts' pivot rows
}
template <class S>
__global__ __launch_bounds__(256) void mf_scatter_out_kernel(const int32_t* perm, const S* x, S* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[perm[i]] = x[i];
}

// forward: fronts list[0 .. gridDim.x) of one height.  LDS: r (ns), y (ns), acc (ms).
template <class S>
__device__ __forceinline__ void mf_fwd_front(const MfFront f, unsigned char* lds_raw, const MfFront* fr,
                                             const int32_t* chl, const S* F, const int32_t* cmap, const int32_t* pinv,
                                             S* w, S* u) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int d = f.d, ns = f.ns, ms = f.ms;
    S* r = reinterpret_cast<S*>(lds_raw);
    S* y = r + ns;
    S* acc = y + ns;
    // up to KC children: every child's header, its first 256 (position, value) pairs and this
    // thread's pivot index are loaded before anything waits on them (one chain of dependent loads
    // instead of one per child); the contributions are then applied child by child in the fixed
    // order, as before
    constexpr int KC = 4;
    const int nch = f.ch1 - f.ch0;
    const bool pre = nch <= KC;
    int cms[KC], cpos[KC];
    const int32_t* cmp[KC];
    const S* cup[KC];
    S cval[KC];
    if (pre) {
#pragma unroll
        for (int q = 0; q < KC; ++q)
            if (q < nch) {
                const MfFront c = fr[chl[f.ch0 + q]];
                cms[q] = c.ms;
                cmp[q] = cmap + c.sof;
                cup[q] = u + c.uoff;
            }
#pragma unroll
        for (int q = 0; q < KC; ++q)
            if (q < nch && tid < cms[q]) {
                cpos[q] = cmp[q][tid];
                cval[q] = cup[q][tid];
            }
    }
    const int pv = tid < ns ? pinv[f.c0 + tid] : 0;
    for (int t = tid; t < ns; t += 256) r[t] = w[f.c0 + t];
    for (int t = tid; t < ms; t += 256) acc[t] = s_zero<S>();
    __syncthreads();
    auto apply = [&](int pos, S v) {
        if (pos < ns) r[pos] = sub(r[pos], v);
        else acc[pos - ns] = add(acc[pos - ns], v);
    };
    if (pre) {
#pragma unroll
        for (int q = 0; q < KC; ++q)
            if (q < nch) {
                if (tid < cms[q]) apply(cpos[q], cval[q]);
                for (int t = tid + 256; t < cms[q]; t += 256) apply(cmp[q][t], cup[q][t]);
                __syncthreads();
            }
    } else {
        for (int k = f.ch0; k < f.ch1; ++k) {
            const MfFront c = fr[chl[k]];
            const int32_t* map = cmap + c.sof;
            const S* uc = u + c.uoff;
            for (int t = tid; t < c.ms; t += 256) apply(map[t], uc[t]);
            __syncthreads();
        }
    }
    if (tid < ns) y[tid] = r[pv];
    for (int t = tid + 256; t < ns; t += 256) y[t] = r[pinv[f.c0 + t]];
    __syncthreads();
    if (f.goff >= 0) {
        // one product over the d rows, tpr threads per row (columns interleaved), partials summed
        // in a fixed order
        const S* G = F + f.goff;
        if (d > 128) {   // one thread per row
            for (int i = tid; i < d; i += 256) {
                S v = s_zero<S>();
                const S* Gi = G + i;
                const int jn = i < ns ? i + 1 : ns;   // inv(L11) is lower triangular: skip its zeros
#pragma unroll kMfUnroll
                for (int j = 0; j < jn; ++j) v = add(v, mul(Gi[(int64_t)j * d], y[j]));
                if (i < ns) w[f.c0 + i] = v;
                else u[f.uoff + i - ns] = add(acc[i - ns], v);
            }
            return;
        }
        S* part = acc + ms;
        const int R = d <= 64 ? 64 : 128, tpr = 256 / R;
        const int i = tid % R, p = tid / R;
        S sacc = s_zero<S>();
        if (i < d) {
            const S* Gi = G + i;
            const int jn = i < ns ? i + 1 : ns;   // inv(L11) is lower triangular: skip its zeros
#pragma unroll kMfUnroll
            for (int j = p; j < jn; j += tpr) sacc = add(sacc, mul(Gi[(int64_t)j * d], y[j]));
        }
        part[p * R + i] = sacc;
        __syncthreads();
        if (tid < d) {
            S v = part[tid];
            for (int q = 1; q < tpr; ++q) v = add(v, part[q * R + tid]);
            if (tid < ns) w[f.c0 + tid] = v;
            else u[f.uoff + tid - ns] = add(acc[tid - ns], v);
        }
        return;
    }
    const S* A = F + f.off;
    for (int jb = 0; jb < ns; jb += 64) {
        const int bw = min(64, ns - jb);
        if (wv == 0) {
            S v = lane < bw ? y[jb + lane] : s_zero<S>();
            const int row = jb + min(lane, bw - 1);
            for (int j0 = 0; j0 < bw; j0 += 16) {
                S lv[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) lv[t] = A[row + (int64_t)(jb + min(j0 + t, bw - 1)) * d];
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int j = j0 + t;
                    if (j < bw) {
                        const S yj = mf_rl(v, j);
                        if (lane > j) v = sub(v, mul(lv[t], yj));
                    }
                }
            }
            if (lane < bw) y[jb + lane] = v;
        }
        __syncthreads();
        for (int i = jb + bw + tid; i < d; i += 256) {
            S s = s_zero<S>();
            const S* Ai = A + i + (int64_t)jb * d;
            for (int j0 = 0; j0 < bw; j0 += 16) {
                S lv[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) lv[t] = Ai[(int64_t)min(j0 + t, bw - 1) * d];
#pragma unroll
                for (int t = 0; t < 16; ++t)
                    if (j0 + t < bw) s = add(s, mul(lv[t], y[jb + j0 + t]));
            }
            if (i < ns) y[i] = sub(y[i], s);
            else acc[i - ns] = add(acc[i - ns], s);
        }
        __syncthreads();
    }
    for (int t = tid; t < ns; t += 256) w[f.c0 + t] = y[t];
    for (int t = tid; t < ms; t += 256) u[f.uoff + t] = acc[t];
}

template <class S>
__global__ __launch_bounds__(256) void mf_fwd_kernel(const MfFront* fr, const int32_t* list, const int32_t* chl,
                                                     const S* F, const int32_t* cmap, const int32_t* pinv, S* w,
                                                     S* u) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    mf_fwd_front<S>(fr[list[blockIdx.x]], lds_raw, fr, chl, F, cmap, pinv, w, u);
}

// backward: fronts list[0 .. gridDim.x) of one height (their ancestors solved).  LDS: t (ns), xs (ms).
template <class S>
__device__ __forceinline__ void mf_bwd_front(const MfFront f, unsigned char* lds_raw, const S* F,
                                             const int32_t* sidx, const S* w, S* x) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int d = f.d, ns = f.ns, ms = f.ms;
    S* t = reinterpret_cast<S*>(lds_raw);
    S* xs = t + ns;
    const S w0 = tid < ns ? w[f.c0 + tid] : s_zero<S>();   // issued before the struct gather waits
    for (int q = tid; q < ms; q += 256) xs[q] = x[sidx[f.sof + q]];
    if (f.goff >= 0) {
        // x(pivots) = [inv(U11), -inv(U11) U12] [w(pivots); x(struct)]: wave p takes columns p, p + 4, ...
        if (tid < ns) t[tid] = w0;
        for (int q = tid + 256; q < ns; q += 256) t[q] = w[f.c0 + q];
        __syncthreads();
        const S* G = F + f.goff + (int64_t)d * ns;
        S* part = xs + ms;
        const int k = lane, p = wv;
        S sacc = s_zero<S>();
        if (k < ns) {
            const S* Gk = G + k;
            // inv(U11) is upper triangular: columns from k on (the first of them congruent to p mod 4)
            const int c0 = k > p ? p + ((k - p + 3) / 4) * 4 : p;
#pragma unroll kMfUnroll
            for (int c = c0; c < d; c += 4) sacc = add(sacc, mul(Gk[(int64_t)c * ns], c < ns ? t[c] : xs[c - ns]));
        }
        part[p * 64 + k] = sacc;
        __syncthreads();
        if (tid < ns) x[f.c0 + tid] = add(add(add(part[tid], part[64 + tid]), part[128 + tid]), part[192 + tid]);
        return;
    }
    __syncthreads();
    const S* A = F + f.off;
    for (int k = tid; k < ns; k += 256) {
        S s = s_zero<S>();
        const S* Ak = A + k + (int64_t)ns * d;
        int q0 = 0;
        for (; q0 + 8 <= ms; q0 += 8) {
            S uv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) uv[e] = Ak[(int64_t)(q0 + e) * d];
#pragma unroll
            for (int e = 0; e < 8; ++e) s = add(s, mul(uv[e], xs[q0 + e]));
        }
        for (; q0 < ms; ++q0) s = add(s, mul(Ak[(int64_t)q0 * d], xs[q0]));
        t[k] = sub(w[f.c0 + k], s);
    }
    __syncthreads();
    for (int jb = ((ns - 1) / 64) * 64; jb >= 0; jb -= 64) {
        const int bw = min(64, ns - jb);
        if (wv == 0) {
            S v = lane < bw ? t[jb + lane] : s_zero<S>();
            const int row = jb + min(lane, bw - 1);
            for (int j1 = bw; j1 > 0; j1 -= 16) {
                S uv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) uv[e] = A[row + (int64_t)(jb + max(j1 - 1 - e, 0)) * d];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = j1 - 1 - e;
                    if (j >= 0) {
                        if (lane == j) v = sdiv(v, uv[e]);
                        const S xj = mf_rl(v, j);
                        if (lane < j) v = sub(v, mul(uv[e], xj));
                    }
                }
            }
            if (lane < bw) t[jb + lane] = v;
        }
        __syncthreads();
        for (int i = tid; i < jb; i += 256) {
            S s = s_zero<S>();
            const S* Ai = A + i + (int64_t)jb * d;
            for (int j0 = 0; j0 < bw; j0 += 16) {
                S uv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) uv[e] = Ai[(int64_t)min(j0 + e, bw - 1) * d];
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (j0 + e < bw) s = add(s, mul(uv[e], t[jb + j0 + e]));
            }
            t[i] = sub(t[i], s);
        }
        __syncthreads();
    }
    for (int k = tid; k < ns; k += 256) x[f.c0 + k] = t[k];
}

template <class S>
__global__ __launch_bounds__(256) void mf_bwd_kernel(const MfFront* fr, const int32_t* list, const S* F,
                                                     const int32_t* sidx, const S* w, S* x) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    mf_bwd_front<S>(fr[list[blockIdx.x]], lds_raw, F, sidx, w, x);
}

// ---- large fronts: one workgroup per 64-row block, sync-free (the dense path's blocked TRSV,
// dense_lu.hip dense_trsv_kernel, on a front).  Pivot block k of a front publishes its solved 64
// values with write-through stores and raises flag[flag0 + k] to the solve's epoch; a row block
// waits for the flags of the blocks it multiplies.  Blocks a row block waits for have lower
// workgroup indices (forward: ascending pivot blocks, then the struct rows; backward: descending),
// and the launches are small (hundreds of workgroups, all resident), so every wait ends.
// back-off: short sleeps (the chain's hand-off latency is what a solve waits on; the pollers are
// a few hundred workgroups), or the dense TRSV's growing sleeps (EIGSOL_MF_BACKOFF=1)
__device__ __forceinline__ void mf_wait(const int32_t* f, int32_t epoch, int32_t* err, int bo) {
    int spins = 0;
    for (;;) {
        const int32_t v = (bo & 2) ? __hip_atomic_load(const_cast<int32_t*>(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                   : __hip_atomic_load(const_cast<int32_t*>(f), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (v == epoch) break;
        if (!(bo & 1)) __builtin_amdgcn_s_sleep(1);
        else if (spins < 4) __builtin_amdgcn_s_sleep(2);
        else if (spins < 16) __builtin_amdgcn_s_sleep(8);
        else __builtin_amdgcn_s_sleep(32);
        if (++spins > (1 << 24)) { atomicOr(err, 1); break; }
    }
}

// z (d entries per large front) = the permuted pivot right-hand side, then the children's
// contributions to the struct rows; one workgroup per front.  LDS: r (ns)
template <class S>
__device__ __forceinline__ void mf_big_asm_front(const MfFront& f, unsigned char* lds_raw, const MfFront* fr,
                                                 const int32_t* chl, const int32_t* cmap, const int32_t* pinv, S* w,
                                                 const S* u, S* z, int bo) {
    const int tid = threadIdx.x, ns = f.ns, ms = f.ms;
    S* r = reinterpret_cast<S*>(lds_raw);
    S* zs = z + f.zoff;
    for (int t = tid; t < ns; t += 256) r[t] = w[f.c0 + t];
    for (int t = tid; t < ms; t += 256) zs[ns + t] = s_zero<S>();
    __syncthreads();
    for (int k = f.ch0; k < f.ch1; ++k) {
        const MfFront c = fr[chl[k]];
        const int32_t* map = cmap + c.sof;
        const S* uc = u + c.uoff;
        for (int t = tid; t < c.ms; t += 256) {
            const int pos = map[t];
            const S v = uc[t];
            if (pos < ns) r[pos] = sub(r[pos], v);
            else zs[pos] = add(zs[pos], v);   // each position once per child: no race
        }
        __syncthreads();
    }
    for (int t = tid; t < ns; t += 256) zs[t] = r[pinv[f.c0 + t]];
    // value flags: the pivot rows' w (read above, before the barrier) becomes "unsolved" for
    // mf_big_fwd_kernel, the next launch
    if (bo & 4)
        for (int t = tid; t < ns; t += 256) mf_st(w + f.c0 + t, mf_sent(s_zero<S>()));
}

template <class S>
__global__ __launch_bounds__(256) void mf_big_asm_kernel(const MfFront* fr, const int32_t* list, const int32_t* chl,
                                                         const int32_t* cmap, const int32_t* pinv, S* w,
                                                         const S* u, S* z, int bo) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    mf_big_asm_front<S>(fr[list[blockIdx.x]], lds_raw, fr, chl, cmap, pinv, w, u, z, bo);
}

// mf_big_asm_front for mf_fwd_height_kernel: the pivot right-hand side read from b through perm (the
// gather left these rows of w unsolved), the struct rows summed in LDS too, and every z entry stored
// once with its value as its flag.  The same sums in the same order.  LDS: r (d)
template <class S>
__device__ __forceinline__ void mf_big_asm_front2(const MfFront& f, unsigned char* lds_raw, const MfFront* fr,
                                                  const int32_t* chl, const int32_t* cmap, const int32_t* pinv,
                                                  const int32_t* perm, const S* bin, const S* u, S* z) {
    const int tid = threadIdx.x, ns = f.ns, ms = f.ms;
    S* r = reinterpret_cast<S*>(lds_raw);
    for (int t = tid; t < ns; t += 256) r[t] = bin[perm[f.c0 + t]];
    for (int t = tid; t < ms; t += 256) r[ns + t] = s_zero<S>();
    __syncthreads();
    for (int k = f.ch0; k < f.ch1; ++k) {
        const MfFront c = fr[chl[k]];
        const int32_t* map = cmap + c.sof;
        const S* uc = u + c.uoff;
        for (int t = tid; t < c.ms; t += 256) {
            const int pos = map[t];
            const S v = uc[t];
            if (pos < ns) r[pos] = sub(r[pos], v);
            else r[pos] = add(r[pos], v);   // each position once per child: no race
        }
        __syncthreads();
    }
    S* zs = z + f.zoff;
    for (int t = tid; t < ns; t += 256) mf_st(zs + t, mf_clean(r[pinv[f.c0 + t]]));
    for (int t = tid; t < ms; t += 256) mf_st(zs + ns + t, mf_clean(r[ns + t]));
}

// one launch for a height's small fronts (workgroups [0, nsmall): mf_fwd_kernel) and its large fronts'
// assembly (the rest: mf_big_asm_kernel); list = the small fronts, then the large ones.  They touch
// disjoint rows of w and read only lower heights' contributions, so they need no order between them.
template <class S>
__global__ __launch_bounds__(256) void mf_fwd_asm_kernel(const MfFront* fr, const int32_t* list, int32_t nsmall,
                                                         const int32_t* chl, const S* F, const int32_t* cmap,
                                                         const int32_t* pinv, S* w, S* u, S* z, int bo) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const MfFront f = fr[list[blockIdx.x]];
    if ((int32_t)blockIdx.x < nsmall) mf_fwd_front<S>(f, lds_raw, fr, chl, F, cmap, pinv, w, u);
    else mf_big_asm_front<S>(f, lds_raw, fr, chl, cmap, pinv, w, u, z, bo);
}

template <class S>
__device__ __forceinline__ S mf_rls(S v, int j) { return mf_rl(v, j); }

// scalars per pivot block of the large fronts in Tinv: inv(L_kk), inv(U_kk) (mf_inv_kernel), then the
// premultiplied next-to-diagonal tiles inv(L_kk) L_{k,k-1}, inv(U_kk) U_{k,k+1} (mf_premul_kernel)
constexpr int kMfTinv = 16384;

// Inverted diagonal blocks of the large fronts (one workgroup per pivot block, after the
// factorization): Tinv + kMfTinv k holds inv(L_kk) (unit lower), then inv(U_kk), 64 x 64 column-major,
// the identity past a partial block's rn rows.  The solves then apply a diagonal block as a
// 64 x 64 product split over the four waves instead of a 64-step dependent chain on one wave.
template <class S>
__global__ __launch_bounds__(256) void mf_inv_kernel(const MfFront* fr, const int32_t* tab, const S* F, S* Tinv) {
    __shared__ S T[64 * 65];
    __shared__ S X[64 * 65];
    const int s = tab[2 * blockIdx.x], k = tab[2 * blockIdx.x + 1];
    const MfFront f = fr[s];
    const int tid = threadIdx.x, d = f.d;
    const int r0 = 64 * k, rn = min(64, f.ns - r0);
    const S* A = F + f.off;
    S one;
    set_re_im(one, 1.0, 0.0);
    for (int e = tid; e < 64 * 64; e += 256) {
        const int i = e & 63, j = e >> 6;
        T[i + j * 65] = (i < rn && j < rn) ? A[(r0 + i) + (int64_t)(r0 + j) * d] : (i == j ? one : s_zero<S>());
    }
    __syncthreads();
    S* out = Tinv + (int64_t)(f.flag0 + k) * kMfTinv;
    // inv(L): thread t < 64 solves column t by forward substitution (unit diagonal)
    if (tid < 64) {
        const int t = tid;
        for (int i = 0; i < 64; ++i) {
            S v = i == t ? one : s_zero<S>();
            for (int j = t; j < i; ++j) v = sub(v, mul(T[i + j * 65], X[j + t * 65]));
            X[i + t * 65] = i < t ? s_zero<S>() : v;
        }
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) out[e] = X[(e & 63) + (e >> 6) * 65];
    __syncthreads();
    // inv(U): back substitution, column t
    if (tid < 64) {
        const int t = tid;
        for (int i = 63; i >= 0; --i) {
            S v = i == t ? one : s_zero<S>();
            for (int j = i + 1; j <= t; ++j) v = sub(v, mul(T[i + j * 65], X[j + t * 65]));
            X[i + t * 65] = i > t ? s_zero<S>() : sdiv(v, T[i + i * 65]);
        }
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) out[4096 + e] = X[(e & 63) + (e >> 6) * 65];
}

// Inverse form of a one-workgroup front with at most 64 pivots (after the factorization;
// EIGSOL_MF_INVFORM=0: off; at most 256 rows): the
// forward solve of the front becomes one product [inv(L11); L21 inv(L11)] (P r) and the backward one
// [inv(U11), -inv(U11) U12] [t; x(struct)], every load independent, instead of a dependent chain
// over the pivot columns on one wave followed by the struct rows (the diagonal blocks of the large
// fronts are inverted the same way, mf_inv_kernel).
template <class S>
__global__ __launch_bounds__(256) void mf_invform2_kernel(const MfFront* fr, const int32_t* list, S* F) {
    // Built for latency (the first kernel, one HBM load per multiply-add, gave bitwise the same forms):
    // inv(L11) (wave 0) and inv(U11) (wave 1) concurrently into one LDS array X (strictly below the
    // diagonal inv(L11), whose unit diagonal is implicit; on and above it inv(U11)), and L21 / U12 read
    // from HBM once, 64-row / 64-column tiles staged in T (free after the inversions).
    __shared__ S T[64 * 65];
    __shared__ S X[64 * 65];
    const MfFront f = fr[list[blockIdx.x]];
    const int tid = threadIdx.x, d = f.d, ns = f.ns, wv = tid >> 6, lane = tid & 63;
    const S* A = F + f.off;
    S* Gf = F + f.goff;
    S* Gb = Gf + (int64_t)d * ns;
    S one;
    set_re_im(one, 1.0, 0.0);
    for (int e = tid; e < 64 * 64; e += 256) {
        const int i = e & 63, j = e >> 6;
        T[i + j * 65] = (i < ns && j < ns) ? A[i + (int64_t)j * d] : (i == j ? one : s_zero<S>());
    }
    __syncthreads();
    // XL(k, j): inv(L11) with its implicit unit diagonal and the zeros above it
    auto xl = [&](int k, int j) { return k == j ? one : (k < j ? s_zero<S>() : X[k + j * 65]); };
    if (wv == 0) {   // inv(L11), column t (unit lower)
        const int t = lane;
        for (int i = t + 1; i < 64; ++i) {
            S v = s_zero<S>();
            for (int j = t; j < i; ++j) v = sub(v, mul(T[i + j * 65], xl(j, t)));
            X[i + t * 65] = v;
        }
    } else if (wv == 1) {   // inv(U11), column t
        const int t = lane;
        for (int i = t; i >= 0; --i) {
            S v = i == t ? one : s_zero<S>();
            for (int j = i + 1; j <= t; ++j) v = sub(v, mul(T[i + j * 65], X[j + t * 65]));
            X[i + t * 65] = sdiv(v, T[i + i * 65]);
        }
    }
    __syncthreads();
    // rows < ns of the forward form: inv(L11)
    for (int e = tid; e < ns * ns; e += 256) {
        const int i = e % ns, j = e / ns;
        Gf[i + (int64_t)j * d] = xl(i, j);
    }
    // columns < ns of the backward form: inv(U11)
    for (int e = tid; e < ns * ns; e += 256) {
        const int i = e % ns, c = e / ns;
        Gb[i + (int64_t)c * ns] = i <= c ? X[i + c * 65] : s_zero<S>();
    }
    // W = L21 inv(L11), 64 rows of L21 at a time through T
    for (int i0 = ns; i0 < d; i0 += 64) {
        const int rn = min(64, d - i0);
        __syncthreads();
        for (int e = tid; e < 64 * ns; e += 256) {
            const int i = e & 63, k = e >> 6;
            if (i < rn) T[i + k * 65] = A[(i0 + i) + (int64_t)k * d];
        }
        __syncthreads();
        for (int e = tid; e < rn * ns; e += 256) {
            const int i = e % rn, j = e / rn;
            S v = s_zero<S>();
            for (int k = j; k < ns; ++k) v = add(v, mul(T[i + k * 65], xl(k, j)));
            Gf[(i0 + i) + (int64_t)j * d] = v;
        }
    }
    // -inv(U11) U12, 64 columns of U12 at a time through T
    for (int c0 = ns; c0 < d; c0 += 64) {
        const int cn = min(64, d - c0);
        __syncthreads();
        for (int e = tid; e < ns * 64; e += 256) {
            const int k = e % ns, c = e / ns;
            if (c < cn) T[k + c * 65] = A[k + (int64_t)(c0 + c) * d];
        }
        __syncthreads();
        for (int e = tid; e < ns * cn; e += 256) {
            const int i = e % ns, c = e / ns;
            S v = s_zero<S>();
            for (int k = i; k < ns; ++k) v = sub(v, mul(X[i + k * 65], T[k + c * 65]));
            Gb[i + (int64_t)(c0 + c) * ns] = v;
        }
    }
}


// The premultiplied next-to-diagonal tiles of the large fronts' row-block solves (bo & 8), one
// workgroup per pivot block after mf_inv_kernel: Tinv + kMfTinv k + 8192 = inv(L_kk) L_{k,k-1} (k >= 1;
// rows past a partial block zero), + 12288 = inv(U_kk) U_{k,k+1} (k <= nblk - 2; columns past a partial
// next block zero), 64 x 64 column-major.  Thread = one column, 16 rows.
template <class S>
__global__ __launch_bounds__(256) void mf_premul_kernel(const MfFront* fr, const int32_t* tab, const S* F, S* Tinv) {
    __shared__ S ti[64 * 65];
    __shared__ S tl[64 * 65];
    const int s = tab[2 * blockIdx.x], k = tab[2 * blockIdx.x + 1];
    const MfFront f = fr[s];
    const int tid = threadIdx.x, d = f.d, ns = f.ns;
    const int nblk = (ns + 63) / 64;
    const int r0 = 64 * k, rn = min(64, ns - r0);
    const S* A = F + f.off;
    S* base = Tinv + (int64_t)(f.flag0 + k) * kMfTinv;
    for (int up = 0; up < 2; ++up) {
        S* out = base + 8192 + 4096 * up;
        const int c = up ? k + 1 : k - 1;
        if (c < 0 || c >= nblk) {
            for (int e = tid; e < 4096; e += 256) out[e] = s_zero<S>();
            continue;
        }
        const int c0 = 64 * c, cn = min(64, ns - c0);
        __syncthreads();
        for (int e = tid; e < 4096; e += 256) {
            const int i = e & 63, j = e >> 6;
            ti[i + j * 65] = base[4096 * up + e];
            tl[i + j * 65] = (i < rn && j < cn) ? A[(r0 + i) + (int64_t)(c0 + j) * d] : s_zero<S>();
        }
        __syncthreads();
        const int j = tid & 63, i0 = (tid >> 6) * 16;
        S o[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) o[t] = s_zero<S>();
        for (int q = 0; q < 64; ++q) {
            const S b = tl[q + j * 65];
#pragma unroll
            for (int t = 0; t < 16; ++t) o[t] = add(o[t], mul(ti[(i0 + t) + q * 65], b));
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) out[(i0 + t) + j * 64] = o[t];
    }
}

// acc += tile(row, c0 .. c0 + 16) * yv over the columns below lim (tile values already loaded)
template <class S>
__device__ __forceinline__ void mf_acc16(S& acc, const S (&tv)[16], const S* yv, int c0, int lim) {
#pragma unroll
    for (int t = 0; t < 16; ++t)
        if (c0 + t < lim) acc = add(acc, mul(tv[t], yv[t]));
}

// forward, large fronts: tab = (front, row block) pairs; row block k < nblk: pivot rows
// [64 k, 64 k + 64) (applies inv(L_kk), publishes, raises the flag); k >= nblk: struct rows (their
// contribution u = children's part + L21 y).  Every wave takes 16 columns of each column block:
// its tile values are loaded before the block's flag is awaited.
template <class S>
__device__ __forceinline__ void mf_big_fwd_block(const int bid, const MfFront* fr, const int32_t* tab, const S* F,
                                                 const S* Tinv, S* z, S* w, S* u, int32_t* flag, int32_t epoch,
                                                 int32_t* err, int bo, S* x, const bool zpoll) {
    __shared__ S part[4][64];
    __shared__ S ysh[4][16];
    __shared__ S vsh[64];
    const int s = tab[2 * bid], rb = tab[2 * bid + 1];
    const MfFront f = fr[s];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int d = f.d, ns = f.ns;
    const int nblk = (ns + 63) / 64;
    const bool piv = rb < nblk;
    const int r0 = piv ? 64 * rb : ns + 64 * (rb - nblk);
    const int rn = min(64, (piv ? ns : d) - r0);
    const S* A = F + f.off;
    const int row = r0 + min(lane, rn - 1);
    S iv[16];
    if (piv) {
        const S* ti = Tinv + (int64_t)(f.flag0 + rb) * kMfTinv + lane + (16 * wv) * 64;
#pragma unroll
        for (int t = 0; t < 16; ++t) iv[t] = ti[t * 64];
    }
    S acc = s_zero<S>();
    // the assembled right-hand side of these rows, loaded before the chain of waits (it was a
    // dependent round trip after the last one, on every hand-off's critical path)
    // zpoll (mf_fwd_height_kernel): z is assembled in this launch and value-flagged; wave 0 polls it after
    // the chain and hands the slot back to the sentinel (this workgroup is its only reader)
    S zr = (!zpoll && lane < rn) ? z[f.zoff + r0 + lane] : s_zero<S>();
    // bo & 8 (value flags only): block rb - 1 enters last, as a product with the premultiplied tile
    // inv(L_rr) L_{r,r-1} after y' = inv(L_rr) (z - the other blocks), so a hand-off is followed by one
    // 64 x 64 product instead of two
    const bool premul = (bo & 12) == 12 && piv && rb >= 1;
    const int cend = piv ? (premul ? rb - 1 : rb) : nblk;
    for (int c = 0; c < cend; ++c) {
        const int c0 = 64 * c + 16 * wv;
        S tv[16];
        const S* tile = A + row;
#pragma unroll
        for (int t = 0; t < 16; ++t) tv[t] = tile[(int64_t)min(c0 + t, ns - 1) * d];
        if (bo & 4) {
            if (lane < 16) ysh[wv][lane] = c0 + lane < ns ? mf_poll(w + f.c0 + c0 + lane, err, bo) : s_zero<S>();
        } else {
            if (lane == 0) mf_wait(flag + f.flag0 + c, epoch, err, bo);
            __builtin_amdgcn_wave_barrier();
            if (!(bo & 2)) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (lane < 16) ysh[wv][lane] = c0 + lane < ns ? mf_ld(w + f.c0 + c0 + lane) : s_zero<S>();
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        mf_acc16(acc, tv, ysh[wv], c0, ns);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    S tm[16];
    S yl = s_zero<S>();
    const int lc0 = 64 * (rb - 1) + 16 * wv;
    if (premul) {
        if (lane < 16) yl = mf_ld(w + f.c0 + lc0 + lane);   // first poll, under the reductions
        const S* tp = Tinv + (int64_t)(f.flag0 + rb) * kMfTinv + 8192 + lane + (16 * wv) * 64;
#pragma unroll
        for (int t = 0; t < 16; ++t) tm[t] = tp[t * 64];
    }
    if (zpoll && wv == 0 && lane < rn) {
        zr = mf_poll(z + f.zoff + r0 + lane, err, bo);
        mf_st(z + f.zoff + r0 + lane, mf_sent(s_zero<S>()));
    }
    part[wv][lane] = acc;
    __syncthreads();
    const S sum = add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane]));
    if (!piv) {
        if (wv == 0 && lane < rn) u[f.uoff + (r0 - ns) + lane] = add(zr, sum);
        return;
    }
    if (wv == 0) vsh[lane] = lane < rn ? sub(zr, sum) : s_zero<S>();
    __syncthreads();
    S p = s_zero<S>();
#pragma unroll
    for (int t = 0; t < 16; ++t) p = add(p, mul(iv[t], vsh[16 * wv + t]));
    part[wv][lane] = p;
    __syncthreads();
    S y = s_zero<S>();
    if (wv == 0) y = add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane]));
    if (premul) {
        __shared__ S part2[4][64];
        if (lane < 16) {
            if (mf_unready(yl)) yl = mf_poll(w + f.c0 + lc0 + lane, err, bo);
            ysh[wv][lane] = yl;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        S q = s_zero<S>();
#pragma unroll
        for (int t = 0; t < 16; ++t) q = add(q, mul(tm[t], ysh[wv][t]));
        part2[wv][lane] = q;
        __syncthreads();
        if (wv == 0) y = sub(y, add(add(part2[0][lane], part2[1][lane]), add(part2[2][lane], part2[3][lane])));
    }
    if (wv != 0) return;
    if (bo & 4) {
        // publish (the value is its own flag); x of these rows becomes "unsolved" for the backward pass
        if (lane < rn) {
            mf_st(w + f.c0 + r0 + lane, mf_clean(y));
            mf_st(x + f.c0 + r0 + lane, mf_sent(y));
        }
        return;
    }
    if (lane < rn) mf_st(w + f.c0 + r0 + lane, y);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(flag + f.flag0 + rb, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

template <class S>
__global__ __launch_bounds__(256) void mf_big_fwd_kernel(const MfFront* fr, const int32_t* tab, const S* F,
                                                         const S* Tinv, S* z, S* w, S* u, int32_t* flag,
                                                         int32_t epoch, int32_t* err, int bo, S* x) {
    mf_big_fwd_block<S>((int)blockIdx.x, fr, tab, F, Tinv, z, w, u, flag, epoch, err, bo, x, false);
}

// One forward launch per height with large fronts (value flags): workgroups [0, nsmall) the small fronts,
// [nsmall, nsmall + nbig) the large fronts' assembly (mf_big_asm_front2: z written once per entry,
// value-flagged), the rest the large fronts' row blocks (mf_big_fwd_block, polling z after their chain).
// Every workgroup waits only on lower-indexed ones; the large fronts' pivot rows of w were set to the
// sentinel by mf_gather_kernel.
template <class S>
__global__ __launch_bounds__(256) void mf_fwd_height_kernel(const MfFront* fr, const int32_t* list, int32_t nsmall,
                                                            int32_t nbig, const int32_t* tab, const int32_t* chl,
                                                            const S* F, const S* Tinv, const int32_t* cmap,
                                                            const int32_t* pinv, const int32_t* perm, const S* bin,
                                                            S* w, S* u, S* z, int32_t* err, int bo, S* x) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int32_t b = (int32_t)blockIdx.x;
    if (b < nsmall) mf_fwd_front<S>(fr[list[b]], lds_raw, fr, chl, F, cmap, pinv, w, u);
    else if (b < nsmall + nbig) mf_big_asm_front2<S>(fr[list[b]], lds_raw, fr, chl, cmap, pinv, perm, bin, u, z);
    else mf_big_fwd_block<S>((int)(b - nsmall - nbig), fr, tab, F, Tinv, z, w, u, nullptr, 0, err, bo, x, true);
}

// backward, large fronts: tab = (front, pivot block) pairs, blocks descending within a front:
// t = y - U12 x(struct) - U[rows, later blocks] x, then inv(U_kk) t (publish, flag)
template <class S>
__device__ __forceinline__ void mf_big_bwd_block(const int bid, const MfFront* fr, const int32_t* tab, const S* F,
                                                 const S* Tinv, const int32_t* sidx, const S* w, S* x,
                                                 int32_t* flag, int32_t epoch, int32_t* err, int bo) {
    __shared__ S part[4][64];
    __shared__ S ysh[4][16];
    __shared__ S vsh[64];
    extern __shared__ __align__(16) unsigned char xs_raw[];
    S* xsh = reinterpret_cast<S*>(xs_raw);   // x(struct), ms entries
    const int s = tab[2 * bid], rb = tab[2 * bid + 1];
    const MfFront f = fr[s];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int d = f.d, ns = f.ns, ms = f.ms;
    const int nblk = (ns + 63) / 64;
    const int r0 = 64 * rb, rn = min(64, ns - r0);
    const S* A = F + f.off;
    const int row = r0 + min(lane, rn - 1);
    S iv[16];
    {
        const S* ti = Tinv + (int64_t)(f.flag0 + rb) * kMfTinv + 4096 + lane + (16 * wv) * 64;
#pragma unroll
        for (int t = 0; t < 16; ++t) iv[t] = ti[t * 64];
    }
    S acc = s_zero<S>();
    const S wr = lane < rn ? w[f.c0 + r0 + lane] : s_zero<S>();   // loaded before the waits (see forward)
    // U12 x(struct): x(struct) (the ancestors' x: earlier launches) gathered into LDS once, then
    // 16-column chunks, wave wv every 4th, two chunks' tiles in flight (the gather and the tile
    // loads used to chain one round trip per chunk: ms = 1000 took ~50 us of a 68 us launch)
    for (int q = tid; q < ms; q += 256) xsh[q] = x[sidx[f.sof + q]];
    __syncthreads();
    {
        const S* tile = A + row + (int64_t)ns * d;
        int q0 = 16 * wv;
        for (; q0 + 64 < ms; q0 += 128) {
            S ta[16], tb[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) ta[t] = tile[(int64_t)(q0 + t) * d];
#pragma unroll
            for (int t = 0; t < 16; ++t) tb[t] = tile[(int64_t)min(q0 + 64 + t, ms - 1) * d];
            mf_acc16(acc, ta, xsh + q0, q0, ms);
            mf_acc16(acc, tb, xsh + q0 + 64, q0 + 64, ms);
        }
        if (q0 < ms) {
            S ta[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) ta[t] = tile[(int64_t)min(q0 + t, ms - 1) * d];
            mf_acc16(acc, ta, xsh + q0, q0, ms);
        }
    }
    // later pivot blocks of this front as their flags rise (the last block first); bo & 8: block rb + 1
    // last, as a product with the premultiplied inv(U_rr) U_{r,r+1} (see the forward block)
    const bool premul = (bo & 12) == 12 && rb + 1 < nblk;
    for (int c = nblk - 1; c > (premul ? rb + 1 : rb); --c) {
        const int c0 = 64 * c + 16 * wv;
        S tv[16];
        const S* tile = A + row;
#pragma unroll
        for (int t = 0; t < 16; ++t) tv[t] = tile[(int64_t)min(c0 + t, ns - 1) * d];
        if (bo & 4) {
            if (lane < 16) ysh[wv][lane] = c0 + lane < ns ? mf_poll(x + f.c0 + c0 + lane, err, bo) : s_zero<S>();
        } else {
            if (lane == 0) mf_wait(flag + f.flag0 + c, epoch, err, bo);
            __builtin_amdgcn_wave_barrier();
            if (!(bo & 2)) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (lane < 16) ysh[wv][lane] = c0 + lane < ns ? mf_ld(x + f.c0 + c0 + lane) : s_zero<S>();
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        mf_acc16(acc, tv, ysh[wv], c0, ns);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    S tm[16];
    S xl = s_zero<S>();
    const int lc0 = 64 * (rb + 1) + 16 * wv;
    if (premul) {
        if (lane < 16 && lc0 + lane < ns) xl = mf_ld(x + f.c0 + lc0 + lane);
        const S* tp = Tinv + (int64_t)(f.flag0 + rb) * kMfTinv + 12288 + lane + (16 * wv) * 64;
#pragma unroll
        for (int t = 0; t < 16; ++t) tm[t] = tp[t * 64];
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0) {
        const S sum = add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane]));
        vsh[lane] = lane < rn ? sub(wr, sum) : s_zero<S>();
    }
    __syncthreads();
    S p = s_zero<S>();
#pragma unroll
    for (int t = 0; t < 16; ++t) p = add(p, mul(iv[t], vsh[16 * wv + t]));
    part[wv][lane] = p;
    __syncthreads();
    S xv = s_zero<S>();
    if (wv == 0) xv = add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane]));
    if (premul) {
        __shared__ S part2[4][64];
        if (lane < 16) {
            if (lc0 + lane < ns) {
                if (mf_unready(xl)) xl = mf_poll(x + f.c0 + lc0 + lane, err, bo);
            } else {
                xl = s_zero<S>();
            }
            ysh[wv][lane] = xl;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        S q = s_zero<S>();
#pragma unroll
        for (int t = 0; t < 16; ++t) q = add(q, mul(tm[t], ysh[wv][t]));
        part2[wv][lane] = q;
        __syncthreads();
        if (wv == 0) xv = sub(xv, add(add(part2[0][lane], part2[1][lane]), add(part2[2][lane], part2[3][lane])));
    }
    if (wv != 0) return;
    if (bo & 4) {
        if (lane < rn) mf_st(x + f.c0 + r0 + lane, mf_clean(xv));
        return;
    }
    if (lane < rn) mf_st(x + f.c0 + r0 + lane, xv);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(flag + f.flag0 + rb, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

template <class S>
__global__ __launch_bounds__(256) void mf_big_bwd_kernel(const MfFront* fr, const int32_t* tab, const S* F,
                                                         const S* Tinv, const int32_t* sidx, const S* w, S* x,
                                                         int32_t* flag, int32_t epoch, int32_t* err, int bo) {
    mf_big_bwd_block<S>((int)blockIdx.x, fr, tab, F, Tinv, sidx, w, x, flag, epoch, err, bo);
}

// one launch for a height's large-front row blocks (workgroups [0, nbb), waiting on each other's values;
// dispatched first) and its small fronts (the rest, mf_bwd_kernel's; they read only their ancestors' x)
template <class S>
__global__ __launch_bounds__(256) void mf_bwd_big_small_kernel(const MfFront* fr, const int32_t* tab, int32_t nbb,
                                                               const int32_t* list, const S* F, const S* Tinv,
                                                               const int32_t* sidx, const S* w, S* x,
                                                               int32_t* flag, int32_t epoch, int32_t* err, int bo) {
    if ((int32_t)blockIdx.x < nbb) {
        mf_big_bwd_block<S>((int)blockIdx.x, fr, tab, F, Tinv, sidx, w, x, flag, epoch, err, bo);
    } else {
        extern __shared__ __align__(16) unsigned char lds_raw[];
        mf_bwd_front<S>(fr[list[blockIdx.x - nbb]], lds_raw, F, sidx, w, x);
    }
}

}  // namespace dev

// ================================================================== host side
struct MfFactor {
    eigsol_ctx* ctx = nullptr;
    int dtype = EIGSOL_F64;
    int64_t n = 0;
    dev::MfFront* fronts = nullptr;
    int32_t* chl = nullptr;
    int32_t* sidx = nullptr;
    int32_t* cmap = nullptr;
    int32_t* perm = nullptr;   // new -> old
    int32_t* pinv = nullptr;   // composite pivot permutation, per front local
    int32_t* lists = nullptr;  // fronts by height, each height's list by descending ns
    void* F = nullptr;
    void* u = nullptr;
    void* w = nullptr;
    void* x = nullptr;
    MfSolveTables T;                  // per height: where its fronts and row blocks are in slists / tabf / tabb
    int32_t* slists = nullptr;
    int32_t* tabf = nullptr;
    int32_t* tabb = nullptr;
    int32_t* flags = nullptr;         // one per pivot block of the large fronts (epoch words)
    int32_t* err = nullptr;           // a flag wait that timed out
    void* z = nullptr;                // large fronts' assembled right-hand sides
    void* tinv = nullptr;             // inverted diagonal blocks of the large fronts and premultiplied tiles (kMfTinv scalars each)
    int32_t epoch = 0;
    int backoff = 2;                  // EIGSOL_MF_BACKOFF: 1 growing sleeps, 2 relaxed polls (flag stores: release)
    bool fuse_asm = true;             // EIGSOL_MF_FUSE_ASM=0: small fronts and large-front assembly as two launches
    bool fuse_big = true;             // EIGSOL_MF_FUSE_BIG=0: no mf_fwd_height_kernel
    uint8_t* bigm = nullptr;          // [n] 1 on the large fronts' pivot rows (mf_fwd_height_kernel's gather)
    MfStats st;
    int64_t nstatic = 0;   // static pivots of the factorization (0 unless the retry set them)
};

void mf_free(MfFactor* f) {
    if (!f) return;
    hipSetDevice(f->ctx->device);
    hipStreamSynchronize(f->ctx->stream);
    for (void* p : {(void*)f->fronts, (void*)f->chl, (void*)f->sidx, (void*)f->cmap, (void*)f->perm, (void*)f->pinv,
                    (void*)f->lists, f->F, f->u, f->w, f->x, (void*)f->slists, (void*)f->tabf, (void*)f->tabb,
                    (void*)f->flags, (void*)f->err, f->z, f->tinv, (void*)f->bigm})
        if (p) hipFree(p);
    ctx_release(f->ctx);
    delete f;
}

const MfStats& mf_stats(const MfFactor* f) { return f->st; }

template <class S>
int mf_create_t(eigsol_ctx* ctx, int dtype, MfHost& X, const S* vals, MfFactor** out, double tau, int64_t* nstatic) {
    *out = nullptr;
    using clk = std::chrono::steady_clock;
    constexpr int NB = dev::RankKMax<S>::value;
    const int64_t sb = (int64_t)sizeof(S);
    if (X.nb != NB || X.sb != sb) return fail(EIGSOL_E_INVALID, "solve_shifted: multifrontal plan of another scalar type");
    const int64_t n = X.n, nnz = X.nnz;
    MfPlan& P = X.P;
    const int64_t nt = P.nt;
    auto& fr = P.fr;
    const auto& chl = P.chl;
    const auto& sidx = P.sidx;
    const auto& lists = P.lists;
    const int32_t H = P.H;
    const double fe = P.fe, fac = P.fac;
    const int64_t uo = P.uo;
    MfStats& stt = X.stt;
    const auto& dst = X.dst;
    const auto &tab = X.tab, &slists = X.slists, &tabf = X.tabf, &tabb = X.tabb;
    const MfSolveTables& T = X.T;
    const int32_t nflag = X.nflag;
    const int64_t zsz = X.zsz;
    // ---- device
    auto* f = new MfFactor();
    f->ctx = ctx;
    ctx_retain(ctx);
    f->dtype = dtype;
    f->n = n;
    f->T = T;
    // the fused forward launch's assembly holds a whole front's right-hand side in LDS
    for (int32_t b : T.lds_asm2)
        if (b > 120 * 1024) f->fuse_big = false;
    if (const char* e = std::getenv("EIGSOL_MF_BACKOFF")) f->backoff = std::atoi(e) & 3;
    if (const char* e = std::getenv("EIGSOL_MF_FUSE_ASM")) f->fuse_asm = std::atoi(e) != 0;
    if (const char* e = std::getenv("EIGSOL_MF_FUSE_BIG"))
        if (std::atoi(e) == 0) f->fuse_big = false;
    // value flags (bit 4; EIGSOL_MF_VALFLAG=0: epoch flags): 1M convection-diffusion 1.657 -> 1.567 ms
    {
        const char* e = std::getenv("EIGSOL_MF_VALFLAG");
        if (!(e && std::atoi(e) == 0)) f->backoff |= 4;
    }
    // the large fronts' row-block solves take their next-to-diagonal block premultiplied (bit 8, with
    // value flags; EIGSOL_MF_PREMUL=0: off)
    {
        const char* e = std::getenv("EIGSOL_MF_PREMUL");
        if (!(e && std::atoi(e) == 0)) f->backoff |= 8;
    }
    hipStream_t st = ctx->stream;
    int rc = EIGSOL_OK;
    int32_t *d_tab = nullptr, *d_piv = nullptr, *d_z = nullptr;
    int64_t* d_dst = nullptr;
    S* d_v = nullptr;
    // an allocation that fails after the plan's free-memory estimate declines the factor
    // (EIGSOL_E_UNSUPPORTED: the caller goes on with ILU(0)); the out-of-memory status is cleared
    auto dm = [&](void** p, size_t bytes) {
        if (rc == EIGSOL_OK && hipMalloc(p, std::max<size_t>(bytes, 16)) != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            rc = fail(EIGSOL_E_UNSUPPORTED,
                      "solve_shifted: multifrontal buffers (" + std::to_string(bytes >> 20) + " MiB) declined");
        }
    };
    dm((void**)&f->fronts, nt * sizeof(dev::MfFront));
    dm((void**)&f->chl, chl.size() * 4);
    dm((void**)&f->sidx, sidx.size() * 4);
    dm((void**)&f->cmap, P.cmap.size() * 4);
    dm((void**)&f->perm, n * 4);
    dm((void**)&f->pinv, n * 4);
    dm((void**)&f->lists, lists.size() * 4);
    dm((void**)&f->slists, slists.size() * 4);
    dm((void**)&f->tabf, tabf.size() * 4);
    dm((void**)&f->tabb, tabb.size() * 4);
    dm((void**)&f->flags, (size_t)nflag * 4);
    dm((void**)&f->err, 4);
    dm(&f->z, (size_t)zsz * sb);
    dm((void**)&f->bigm, (size_t)n);
    dm(&f->tinv, (size_t)nflag * dev::kMfTinv * sb);
    dm(&f->F, ((size_t)fe + (size_t)X.gsz) * sb);
    int32_t* d_inv = nullptr;
    if (!X.inv_list.empty()) dm((void**)&d_inv, X.inv_list.size() * 4);
    dm(&f->u, (size_t)uo * sb);
    dm(&f->w, n * sb);
    dm(&f->x, n * sb);
    dm((void**)&d_tab, tab.size() * 4);
    dm((void**)&d_piv, n * 4);
    dm((void**)&d_z, 8);   // [0] zero-pivot flag, [1] static pivots
    dm((void**)&d_dst, nnz * 8);
    dm((void**)&d_v, nnz * sb);
    std::vector<int32_t> hpiv(n);
    int32_t hz2[2] = {0, 0};
    const int32_t& hz = hz2[0];
    if (rc == EIGSOL_OK) {
        const auto t1 = clk::now();
        auto up = [&](void* d, const void* h, size_t b) {
            if (b) hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, st);
        };
        up(f->fronts, fr.data(), nt * sizeof(dev::MfFront));
        up(f->chl, chl.data(), chl.size() * 4);
        up(f->sidx, sidx.data(), sidx.size() * 4);
        up(f->cmap, P.cmap.data(), P.cmap.size() * 4);
        up(f->perm, P.perm.data(), n * 4);
        up(f->lists, lists.data(), lists.size() * 4);
        up(f->slists, slists.data(), slists.size() * 4);
        up(f->tabf, tabf.data(), tabf.size() * 4);
        up(f->tabb, tabb.data(), tabb.size() * 4);
        hipMemsetAsync(f->flags, 0, std::max<size_t>((size_t)nflag * 4, 4), st);
        {
            // the large fronts' pivot rows (mf_fwd_height_kernel's gather) and an all-unsolved z
            std::vector<uint8_t> bm((size_t)n, 0);
            for (int32_t h = 0; h <= H; ++h)
                for (int64_t t = T.sstart[h] + T.nsmall[h]; t < T.sstart[h + 1]; ++t) {
                    const dev::MfFront& q = fr[slists[t]];
                    for (int32_t r = 0; r < q.ns; ++r) bm[(size_t)q.c0 + r] = 1;
                }
            up(f->bigm, bm.data(), (size_t)n);
            hipMemsetD32Async(static_cast<hipDeviceptr_t>(f->z), 0x7FF4DEADu, std::max<size_t>((size_t)zsz * sb / 4, 1), st);
        }
        hipMemsetAsync(f->err, 0, 4, st);
        up(d_tab, tab.data(), tab.size() * 4);
        if (d_inv) up(d_inv, X.inv_list.data(), X.inv_list.size() * 4);
        up(d_dst, dst.data(), nnz * 8);
        up(d_v, vals, nnz * sb);
        hipMemsetAsync(f->F, 0, (size_t)fe * sb, st);
        hipMemsetAsync(d_z, 0, 8, st);
        S* F = static_cast<S*>(f->F);
        if (nnz)
            hipLaunchKernelGGL((dev::mf_scatter_kernel<S>), dim3((nnz + 255) / 256), dim3(256), 0, st, d_dst, d_v, nnz, F);
        for (const MfLaunch& l : X.plan) {
            if (l.kind == 0)
                hipLaunchKernelGGL((dev::mf_extend_kernel<S>), dim3(l.cnt), dim3(256), 0, st, f->fronts, d_tab + l.off,
                                   f->cmap, F);
            else if (l.kind == 1)
                hipLaunchKernelGGL((dev::mf_panel_kernel<S, NB>), dim3(l.cnt), dim3(256), 0, st, f->fronts,
                                   f->lists + l.off, l.q, F, d_piv, d_z, tau, d_z + 1);
            else
                hipLaunchKernelGGL((dev::mf_gemm_kernel<S, NB>), dim3(l.cnt), dim3(256), 0, st, f->fronts, d_tab + l.off,
                                   l.q, F);
        }
        if (!tabb.empty()) {
            hipLaunchKernelGGL((dev::mf_inv_kernel<S>), dim3(tabb.size() / 2), dim3(256), 0, st, f->fronts, f->tabb, F,
                               static_cast<S*>(f->tinv));
            if ((f->backoff & 12) == 12)
                hipLaunchKernelGGL((dev::mf_premul_kernel<S>), dim3(tabb.size() / 2), dim3(256), 0, st, f->fronts,
                                   f->tabb, F, static_cast<S*>(f->tinv));
        }
        if (d_inv)
            hipLaunchKernelGGL((dev::mf_invform2_kernel<S>), dim3(X.inv_list.size()), dim3(256), 0, st, f->fronts, d_inv, F);
        hipMemcpyAsync(hpiv.data(), d_piv, n * 4, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(hz2, d_z, 8, hipMemcpyDeviceToHost, st);
        if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess)
            rc = fail(EIGSOL_E_HIP, "solve_shifted: multifrontal factorization");
        stt.numeric_seconds = std::chrono::duration<double>(clk::now() - t1).count();
        if (std::getenv("EIGSOL_MF_DEBUG")) std::fprintf(stderr, "[mf] upload + numeric %.3f s\n", stt.numeric_seconds);
    }
    for (void* p : {(void*)d_tab, (void*)d_piv, (void*)d_z, (void*)d_dst, (void*)d_v, (void*)d_inv})
        if (p) hipFree(p);
    if (rc == EIGSOL_OK && hz) rc = fail(EIGSOL_E_SOLVER, "solve_shifted: multifrontal LU met a zero pivot");
    if (nstatic) *nstatic = hz2[1];
    f->nstatic = hz2[1];
    if (rc == EIGSOL_OK) {
        // composite interchange of every front: row t of the factored front is row q[t] of the assembled one
        std::vector<int32_t> pinv(n);
        for (int64_t s = 0; s < nt; ++s) {
            const int32_t c0 = fr[s].c0, ns = fr[s].ns;
            int32_t* qv = pinv.data() + c0;
            for (int32_t t = 0; t < ns; ++t) qv[t] = t;
            for (int32_t k = 0; k < ns; ++k) std::swap(qv[k], qv[hpiv[c0 + k]]);
        }
        if (hipMemcpyAsync(f->pinv, pinv.data(), n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            rc = fail(EIGSOL_E_HIP, "solve_shifted: multifrontal pivots");
    }
    if (rc == EIGSOL_OK) {
        int32_t mx = 0;
        for (int32_t b : T.lds_fwd) mx = std::max(mx, b);
        for (int32_t b : T.lds_bwd) mx = std::max(mx, b);
        for (int32_t b : T.lds_asm) mx = std::max(mx, b);
        if (f->fuse_big)
            for (int32_t b : T.lds_asm2) mx = std::max(mx, b);
        const int32_t mxb = *std::max_element(T.lds_bbig.begin(), T.lds_bbig.end());
        auto lds = [](const void* kernel, int32_t bytes) {
            return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
        };
        if (!lds(reinterpret_cast<const void*>(dev::mf_fwd_kernel<S>), mx) ||
            !lds(reinterpret_cast<const void*>(dev::mf_bwd_kernel<S>), mx) ||
            !lds(reinterpret_cast<const void*>(dev::mf_big_asm_kernel<S>), mx) ||
            !lds(reinterpret_cast<const void*>(dev::mf_fwd_asm_kernel<S>), mx) ||
            !lds(reinterpret_cast<const void*>(dev::mf_fwd_height_kernel<S>), mx) ||
            !lds(reinterpret_cast<const void*>(dev::mf_big_bwd_kernel<S>), mxb) ||
            !lds(reinterpret_cast<const void*>(dev::mf_bwd_big_small_kernel<S>), std::max(mx, mxb)))
            rc = fail(EIGSOL_E_HIP, "solve_shifted: multifrontal solve LDS");
    }
    if (rc != EIGSOL_OK) {
        mf_free(f);
        return rc;
    }
    stt.solve_bytes = fac * (double)sb + 2.0 * (double)uo * (double)sb + 6.0 * (double)n * (double)sb;
    f->st = stt;
    *out = f;
    return EIGSOL_OK;
}

// Every launch of one solve, enqueued on st (direct, or inside a stream capture)
template <class S>
static void mf_solve_enqueue(MfFactor* f, hipStream_t st, const S* b, S* out, int32_t ef, int32_t eb) {
    const int64_t n = f->n;
    const MfSolveTables& T = f->T;
    S* w = static_cast<S*>(f->w);
    S* x = static_cast<S*>(f->x);
    const S* F = static_cast<const S*>(f->F);
    // one forward launch per height with large fronts (mf_fwd_height_kernel; value flags,
    // EIGSOL_MF_FUSE_BIG=0 off): the gather leaves those fronts' pivot rows of w unsolved
    const bool hfuse = f->bigm && f->fuse_big && (f->backoff & 4);
    hipLaunchKernelGGL((dev::mf_gather_kernel<S>), dim3((n + 255) / 256), dim3(256), 0, st, f->perm, b, w, n,
                       hfuse ? f->bigm : (const uint8_t*)nullptr);
    const int32_t H = (int32_t)T.nsmall.size() - 1;
    S* u = static_cast<S*>(f->u);
    S* z = static_cast<S*>(f->z);
    for (int32_t h = 0; h <= H; ++h) {
        const int32_t* L = f->slists + T.sstart[h];
        if (hfuse && T.nbig[h]) {
            hipLaunchKernelGGL((dev::mf_fwd_height_kernel<S>), dim3(T.nsmall[h] + T.nbig[h] + T.fcnt[h]), dim3(256),
                               std::max(T.lds_fwd[h], T.lds_asm2[h]), st, f->fronts, L, (int32_t)T.nsmall[h],
                               (int32_t)T.nbig[h], f->tabf + 2 * T.foff[h], f->chl, F, (const S*)f->tinv, f->cmap,
                               f->pinv, f->perm, b, w, u, z, f->err, f->backoff, x);
            continue;
        }
        // EIGSOL_MF_FUSE_ASM=0: the small fronts and the large fronts' assembly as two launches
        const bool fuse = f->fuse_asm && T.nsmall[h] && T.nbig[h];
        if (fuse)
            hipLaunchKernelGGL((dev::mf_fwd_asm_kernel<S>), dim3(T.nsmall[h] + T.nbig[h]), dim3(256),
                               std::max(T.lds_fwd[h], T.lds_asm[h]), st, f->fronts, L, T.nsmall[h], f->chl, F,
                               f->cmap, f->pinv, w, u, z, f->backoff);
        else if (T.nsmall[h])
            hipLaunchKernelGGL((dev::mf_fwd_kernel<S>), dim3(T.nsmall[h]), dim3(256), T.lds_fwd[h], st, f->fronts,
                               L, f->chl, F, f->cmap, f->pinv, w, u);
        if (T.nbig[h]) {
            if (!fuse)
                hipLaunchKernelGGL((dev::mf_big_asm_kernel<S>), dim3(T.nbig[h]), dim3(256), T.lds_asm[h], st,
                                   f->fronts, L + T.nsmall[h], f->chl, f->cmap, f->pinv, w, (const S*)u, z,
                                   f->backoff);
            hipLaunchKernelGGL((dev::mf_big_fwd_kernel<S>), dim3(T.fcnt[h]), dim3(256), 0, st, f->fronts,
                               f->tabf + 2 * T.foff[h], F, (const S*)f->tinv, z, w, u, f->flags, ef, f->err,
                               f->backoff, x);
        }
    }
    for (int32_t h = H; h >= 0; --h) {
        const int32_t* L = f->slists + T.sstart[h];
        if (f->fuse_asm && T.nbig[h] && T.nsmall[h]) {
            hipLaunchKernelGGL((dev::mf_bwd_big_small_kernel<S>), dim3(T.bcnt[h] + T.nsmall[h]), dim3(256),
                               std::max(T.lds_bbig[h], T.lds_bwd[h]), st, f->fronts, f->tabb + 2 * T.boff[h],
                               T.bcnt[h], L, F, (const S*)f->tinv, f->sidx, (const S*)w, x, f->flags, eb, f->err,
                               f->backoff);
            continue;
        }
        if (T.nbig[h])
            hipLaunchKernelGGL((dev::mf_big_bwd_kernel<S>), dim3(T.bcnt[h]), dim3(256), T.lds_bbig[h], st, f->fronts,
                               f->tabb + 2 * T.boff[h], F, (const S*)f->tinv, f->sidx, (const S*)w, x, f->flags, eb,
                               f->err, f->backoff);
        if (T.nsmall[h])
            hipLaunchKernelGGL((dev::mf_bwd_kernel<S>), dim3(T.nsmall[h]), dim3(256), T.lds_bwd[h], st, f->fronts,
                               L, F, f->sidx, w, x);
    }
    hipLaunchKernelGGL((dev::mf_scatter_out_kernel<S>), dim3((n + 255) / 256), dim3(256), 0, st, f->perm, x, out, n);
}

template <class S>
int mf_solve_t(MfFactor* f, const S* b, S* out) {
    hipStream_t st = f->ctx->stream;
    const int64_t n = f->n;
    if (n == 0) return EIGSOL_OK;
    const int32_t ef = ++f->epoch, eb = ++f->epoch;   // flag words: forward, then backward values
    // The ~50 dependent launches of a solve go to the stream one by one.  Replaying them as one
    // hipGraph per repeated (b, out) pair was tried in round 6 (1M convection-diffusion, two A/B
    // pairs): 1.51 ms per iteration with direct launches, 2.82 / 2.86 ms replayed - the replay
    // serialises the nodes behind more than the stream's own launch gaps.  Removed.
    mf_solve_enqueue<S>(f, st, b, out, ef, eb);
    EIGSOL_HIP(hipGetLastError());
    static const bool dbg = std::getenv("EIGSOL_MF_DEBUG") != nullptr;
    if (dbg) {
        int32_t e = 0;
        EIGSOL_HIP(hipMemcpyAsync(&e, f->err, 4, hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipStreamSynchronize(st));
        std::fprintf(stderr, "[mf] solve epoch %d err %d\n", f->epoch, e);
    }
    return EIGSOL_OK;
}

const int32_t* mf_err_word(const MfFactor* f) { return f->err; }

int mf_create(eigsol_ctx* ctx, int dtype, MfHost* X, const void* v, MfFactor** out, double static_pivot,
              int64_t* nstatic) {
    *out = nullptr;
    if (nstatic) *nstatic = 0;
    try {
        if (dtype == EIGSOL_C128)
            return mf_create_t<cplx>(ctx, dtype, *X, static_cast<const cplx*>(v), out, static_pivot, nstatic);
        if (dtype == EIGSOL_F64)
            return mf_create_t<double>(ctx, dtype, *X, static_cast<const double*>(v), out, static_pivot, nstatic);
    } catch (const std::exception& ex) {
        return fail(EIGSOL_E_UNSUPPORTED, std::string("solve_shifted: multifrontal factor: ") + ex.what());
    }
    return EIGSOL_E_UNSUPPORTED;
}

int mf_solve(MfFactor* f, const void* b, void* x) {
    if (f->dtype == EIGSOL_C128) return mf_solve_t<cplx>(f, static_cast<const cplx*>(b), static_cast<cplx*>(x));
    return mf_solve_t<double>(f, static_cast<const double*>(b), static_cast<double*>(x));
}

}  // namespace eigsol

// Host-only analysis of the multifrontal plan (ordering + symbolic), for tests and tools: perm_out
// (n entries, new -> old) and fronts_out (4 per front: first column, pivots, struct size, parent)
// may be null; stats_out[8] = fronts, heights, max front, max pivots, factor entries, front
// entries, flops (complex scalars if is_complex), 1 if the plan is consistent.
extern "C" int eigsol_mf_analyze(int64_t n, const int32_t* rowptr, const int32_t* colidx, int32_t leaf,
                                 int32_t is_complex, int32_t* perm_out, int32_t* fronts_out, int64_t fronts_cap,
                                 double* stats_out) {
    using namespace eigsol;
    if (n < 0 || n > INT32_MAX - 1 || (n > 0 && (!rowptr || !colidx)) || !stats_out || leaf < 1 ||
        (rowptr && rowptr[0] != 0))
        return fail(EIGSOL_E_INVALID, "eigsol_mf_analyze: bad arguments");
    for (int64_t i = 0; i < n; ++i) {
        if (rowptr[i + 1] < rowptr[i]) return fail(EIGSOL_E_INVALID, "eigsol_mf_analyze: row pointers not monotone");
        for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
            if (colidx[e] < 0 || colidx[e] >= n) return fail(EIGSOL_E_INVALID, "eigsol_mf_analyze: column index out of range");
    }
    try {
        std::vector<int32_t> rp(rowptr, rowptr + n + 1), ci(colidx, colidx + (n ? rowptr[n] : 0));
        MfPlan P;
        const bool ok = mf_plan(n, rp, ci, leaf, is_complex != 0, P);
        stats_out[0] = (double)P.nt;
        stats_out[1] = (double)(P.H + 1);
        stats_out[2] = (double)P.maxd;
        stats_out[3] = (double)P.maxns;
        stats_out[4] = P.fac;
        stats_out[5] = P.fe;
        stats_out[6] = P.flops;
        stats_out[7] = ok ? 1.0 : 0.0;
        if (perm_out && n) std::copy(P.perm.begin(), P.perm.end(), perm_out);
        if (fronts_out) {
            if (fronts_cap < P.nt) return fail(EIGSOL_E_INVALID, "eigsol_mf_analyze: fronts_out too small");
            for (int64_t s = 0; s < P.nt; ++s) {
                fronts_out[4 * s] = P.fr[s].c0;
                fronts_out[4 * s + 1] = P.fr[s].ns;
                fronts_out[4 * s + 2] = P.fr[s].ms;
                fronts_out[4 * s + 3] = P.fr[s].parent;
            }
        }
        return EIGSOL_OK;
    } catch (const std::exception& ex) {
        return fail(EIGSOL_E_INVALID, std::string("eigsol_mf_analyze: ") + ex.what());
    }
}
