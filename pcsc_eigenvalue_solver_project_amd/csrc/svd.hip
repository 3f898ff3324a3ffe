// Thin singular value decomposition of a dense m x n matrix (gfx950; EIGSOL_F64 / EIGSOL_C128) by block
// one-sided Jacobi (Hestenes): A = U diag(s) V^H, k = min(m, n), U m x k, V n x k, s descending.
//
//   0. m < n: the work is done on A^H (svd_load_t transposes) and the roles of U and V are swapped at the end.
//      The matrix is scaled by a power of two so that its largest component lies in [1, 2); s is scaled back.
//      W <- A (m x n, m >= n from here on), V <- I_n where the working V is needed (see svd_host);
//   1. the columns are cut into blocks of width B (32 real, 16 complex: a pair of blocks is RankKMax columns);
//      one sweep visits every unordered pair of blocks once by the round-robin (circle) schedule: nb - 1 steps
//      (nb odd: nb steps, one block idle in each) of floor(nb / 2) disjoint pairs; n <= B is the single pair
//      (block 0, nothing).  All pairs of a step run in the same three launches:
//   2a. svd_gram: G = X^H X of each pair's m x P columns X (P = 2 B) on the fp64 matrix cores.  A workgroup
//      takes 1024 rows, a wave 256 of them, 16 at a time (no LDS on the way: a lane loads four consecutive
//      rows of one column, the k-steps of the MFMA are a permutation of the rows that A and B share).  The
//      four waves' sums are added in wave order in LDS, the workgroups' partials are written separately;
//   2b. svd_pair_jacobi, one workgroup per pair, G and J in LDS: the partials are added in chunk order;
//      tol = sqrt(m) eps; where max_{i != j} |g_ij| / sqrt(g_ii g_jj) <= tol (a zero diagonal entry counts as
//      0) the pair is marked skipped.  Otherwise cyclic two-sided Jacobi on G to the same relative tolerance
//      (every non-zero entry is rotated, so a pair that was worked on is left at rounding level, not just
//      below tol, and the rounding of later steps cannot push it back over the skip test),
//      the P / 2 disjoint rotations of an inner step at once (each thread owns the 2 x 2 blocks that two
//      rotations meet in), t = sign(d) 2 |g| / (|d| + hypot(d, 2 |g|)) (Rutishauser's smaller root, formed so
//      that a tiny |g| cannot overflow), the phase of g taken into the rotation, the rotations accumulated
//      in J.  J is polished by one Newton-Schulz step, J (1.5 I - 0.5 J^H J): without it the norm drift of
//      the accumulated rotations shows in V's orthogonality.  J and the pair's maximum go to the pair's slot;
//   2c. svd_apply: X <- X J in place for W, and for the same columns of V where V is accumulated, on the fp64
//      matrix cores: a wave owns 16 rows, loads them for all P columns, then stores (no barrier; the rows of
//      other waves are never read).  Skipped pairs are not touched;
//   3. after each sweep the host reads the pairs' maxima (one wait per sweep) and stops where none exceeds tol
//      or max_sweeps is reached;
//   4. sigma_j = ||w_j||_2, a stable descending sort on the host, u_j = w_j / sigma_j; a column with sigma_j
//      exactly 0 is completed from the unit vectors e_k in ascending k, each orthogonalised twice against all
//      columns and accepted at norm >= 0.5 (the host loops over such columns one by one: exact zeros are
//      rare); then the phase convention: column j of V has its largest-modulus component (the first on ties)
//      real positive, and U's column the same phase.
// No floating-point atomics; every sum has a fixed order: two calls give the same bits, and W's path does not
// depend on whether V is accumulated.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "mfma_rankk.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

template <class S> struct SvdCfg {
    static constexpr int B = RankKMax<S>::value / 2;   // block width
    static constexpr int P = RankKMax<S>::value;       // columns of a pair
    static constexpr int LD = P + 1;                   // leading dimension of G and J in LDS
};

struct SvdPair {
    int p, q;     // first columns of the two blocks
    int bp, bq;   // their widths (bq == 0: the single block of n <= B)
};

constexpr int kSvdGramRows = 1024;   // rows per workgroup of svd_gram
constexpr int kSvdApplyRows = 256;   // rows per workgroup of svd_apply

// the column of W behind local column c of a pair, -1 past a ragged block's end
__device__ __forceinline__ int svd_col(const SvdPair& pr, int c, int B) {
    if (c < B) return c < pr.bp ? pr.p + c : -1;
    return c - B < pr.bq ? pr.q + (c - B) : -1;
}

__device__ __forceinline__ double sv_conj(double a) { return a; }
__device__ __forceinline__ cplx sv_conj(cplx a) { return cplx{a.re, -a.im}; }
__device__ __forceinline__ double sv_mod(double a) { return fabs(a); }
__device__ __forceinline__ cplx sv_scale(cplx a, double s) { return cplx{a.re * s, a.im * s}; }
__device__ __forceinline__ double sv_scale(double a, double s) { return a * s; }
__device__ __forceinline__ double sv_mod(cplx a) { return hypot(a.re, a.im); }
__device__ __forceinline__ bool sv_nz(double a) { return a != 0.0; }
__device__ __forceinline__ bool sv_nz(cplx a) { return a.re != 0.0 || a.im != 0.0; }
template <class S> __device__ __forceinline__ S sv_from(double re);
template <> __device__ __forceinline__ double sv_from<double>(double re) { return re; }
template <> __device__ __forceinline__ cplx sv_from<cplx>(double re) { return cplx{re, 0.0}; }

// max over the workgroup (256 threads), the same value on every thread
__device__ __forceinline__ double sv_block_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}
// sum over the workgroup (256 threads) in a fixed tree
__device__ __forceinline__ double sv_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// ------------------------------------------------------------------ set-up
// out[2 b], out[2 b + 1]: the largest |component| that block b saw, and whether it saw a non-finite one
__global__ __launch_bounds__(256) void svd_absmax(const double* A, int64_t cnt, double* out) {
    __shared__ double red[256];
    double mx = 0.0, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        const double v = fabs(A[i]);
        if (!(v <= DBL_MAX)) bad = 1.0;
        else mx = fmax(mx, v);
    }
    mx = sv_block_max(mx, red);
    bad = sv_block_max(bad, red);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = mx;
        out[2 * blockIdx.x + 1] = bad;
    }
}

__global__ __launch_bounds__(256) void svd_scale(double* A, int64_t cnt, double sc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) A[i] *= sc;
}

// Out (cols x rows) = sc In^H (In: rows x cols), 32 x 32 tiles through padded LDS
template <class S>
__global__ __launch_bounds__(256) void svd_load_t(int rows, int cols, const S* In, S* Out, double sc) {
    __shared__ S tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    for (int q = ty; q < 32; q += 8) {
        const int i = i0 + tx, j = j0 + q;
        if (i < rows && j < cols) tile[q][tx] = In[i + (int64_t)j * rows];
    }
    __syncthreads();
    for (int q = ty; q < 32; q += 8) {
        const int j = j0 + tx, i = i0 + q;
        if (i < rows && j < cols) Out[j + (int64_t)i * cols] = sv_scale(sv_conj(tile[tx][q]), sc);
    }
}

template <class S>
__global__ __launch_bounds__(256) void svd_set_identity(S* V, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) V[i + (int64_t)i * n] = sv_from<S>(1.0);
}

// ------------------------------------------------------------------ 2a. Gram matrices
template <class S>
__global__ __launch_bounds__(256) void svd_gram(const S* W, int m, const SvdPair* pairs, int nchunk, S* Gpart) {
    constexpr bool kC = std::is_same_v<S, cplx>;
    constexpr int B = SvdCfg<S>::B, P = SvdCfg<S>::P, NT = P / 16;
    __shared__ S Gs[P * P];
    const SvdPair pr = pairs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int rbeg = blockIdx.x * kSvdGramRows + wave * (kSvdGramRows / 4);
    const int rend = min(rbeg + kSvdGramRows / 4, m);
    int64_t coff[NT];
    bool cval[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = svd_col(pr, 16 * t + li, B);
        cval[t] = c >= 0;
        coff[t] = (int64_t)max(c, 0) * m;
    }
    mfma_d4 are[NT][NT], aim[NT][NT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int c = 0; c < NT; ++c) are[a][c] = aim[a][c] = mfma_d4{0, 0, 0, 0};
    // k-step s of a 16-row slab carries row 4 lk + s on the lanes of k index lk, for both operands
    for (int r0 = rbeg; r0 < rend; r0 += 16) {
        S x[NT][4];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = r0 + 4 * lk + s;
                x[t][s] = (cval[t] && row < m) ? W[coff[t] + row] : s_zero<S>();
            }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int c = 0; c < NT; ++c) {
                    // D[i][j] = sum_k conj(X[k][a0 + i]) X[k][c0 + j]
                    are[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(re_of(x[a][s]), re_of(x[c][s]), are[a][c], 0, 0, 0);
                    if constexpr (kC) {
                        are[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(im_of(x[a][s]), im_of(x[c][s]), are[a][c], 0, 0, 0);
                        aim[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(re_of(x[a][s]), im_of(x[c][s]), aim[a][c], 0, 0, 0);
                        aim[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(-im_of(x[a][s]), re_of(x[c][s]), aim[a][c], 0, 0, 0);
                    }
                }
    }
    // the four waves' sums, added in wave order
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int c = 0; c < NT; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = (16 * a + lk + 4 * r) + (16 * c + li) * P;
                        S v;
                        set_re_im(v, are[a][c][r], aim[a][c][r]);
                        Gs[idx] = w == 0 ? v : add(Gs[idx], v);
                    }
        }
        __syncthreads();
    }
    S* out = Gpart + ((int64_t)blockIdx.y * nchunk + blockIdx.x) * (P * P);
    for (int i = threadIdx.x; i < P * P; i += 256) out[i] = Gs[i];
}

// ------------------------------------------------------------------ 2b. Jacobi on a pair's Gram matrix
// (x1, x2) <- (x1, x2) R, R = [c, sw; -conj(sw), c]
template <class S> __device__ __forceinline__ void sv_rot_cols(S& x1, S& x2, double c, S sw) {
    const S n1 = sub(sv_scale(x1, c), mul(sv_conj(sw), x2));
    const S n2 = add(mul(sw, x1), sv_scale(x2, c));
    x1 = n1;
    x2 = n2;
}
// (x1; x2) <- R^H (x1; x2)
template <class S> __device__ __forceinline__ void sv_rot_rows(S& x1, S& x2, double c, S sw) {
    const S n1 = sub(sv_scale(x1, c), mul(sw, x2));
    const S n2 = add(mul(sv_conj(sw), x1), sv_scale(x2, c));
    x1 = n1;
    x2 = n2;
}

// the circle schedule: step s of cnt - 1 (cnt even), pair i of cnt / 2
__host__ __device__ inline void svd_round_robin(int cnt, int s, int i, int* a, int* b) {
    const int r = cnt - 1;
    if (i == 0) {
        *a = r;
        *b = s % r;
    } else {
        *a = (s + i) % r;
        *b = (s - i + r) % r;
    }
}

template <class S> constexpr size_t svd_jacobi_lds() {
    return 2 * (size_t)SvdCfg<S>::P * SvdCfg<S>::LD * sizeof(S) + (size_t)SvdCfg<S>::P * 8 +
           (size_t)(SvdCfg<S>::P / 2) * (8 + sizeof(S) + 8) + 256 * 8;
}

// max_{a != c} |g_ac| / (sqrt(g_aa) sqrt(g_cc)), a zero diagonal entry counting as 0; dg receives sqrt(g_aa)
template <class S>
__device__ __forceinline__ double svd_offmax(const S* G, double* dg, double* red) {
    constexpr int P = SvdCfg<S>::P, LD = SvdCfg<S>::LD;
    __syncthreads();
    if ((int)threadIdx.x < P) dg[threadIdx.x] = sqrt(fmax(re_of(G[threadIdx.x * (LD + 1)]), 0.0));
    __syncthreads();
    double mx = 0.0;
    for (int idx = threadIdx.x; idx < P * P; idx += 256) {
        const int a = idx % P, c = idx / P;
        const double d = dg[a] * dg[c];
        if (a != c && d > 0.0) mx = fmax(mx, sv_mod(G[a + c * LD]) / d);
    }
    return sv_block_max(mx, red);
}

template <class S>
__global__ __launch_bounds__(256) void svd_pair_jacobi(const S* Gpart, int nchunk, double tol, int max_inner, S* Jout,
                                                       double* pmax, int* pflag) {
    constexpr int P = SvdCfg<S>::P, LD = SvdCfg<S>::LD, HP = P / 2;
    extern __shared__ __align__(16) unsigned char svd_lds[];
    S* G = reinterpret_cast<S*>(svd_lds);
    S* J = G + P * LD;
    S* rsw = J + P * LD;                                   // HP: s w of each rotation
    double* dg = reinterpret_cast<double*>(rsw + HP);      // P
    double* rc = dg + P;                                   // HP
    double* red = rc + HP;                                 // 256
    int* rpq = reinterpret_cast<int*>(red + 256);          // 2 HP
    const int pair = blockIdx.x, tid = threadIdx.x;
    const S* gp = Gpart + (int64_t)pair * nchunk * (P * P);
    for (int idx = tid; idx < P * P; idx += 256) {
        S acc = gp[idx];
        for (int ch = 1; ch < nchunk; ++ch) acc = add(acc, gp[(int64_t)ch * (P * P) + idx]);
        const int a = idx % P, c = idx / P;
        G[a + c * LD] = acc;
        J[a + c * LD] = sv_from<S>(a == c ? 1.0 : 0.0);
    }
    double off = svd_offmax<S>(G, dg, red);
    if (tid == 0) {
        pmax[pair] = off;
        pflag[pair] = off > tol ? 1 : 0;
    }
    if (!(off > tol)) return;
    for (int sweep = 0; sweep < max_inner; ++sweep) {
        for (int step = 0; step < P - 1; ++step) {
            if (tid < HP) {
                int a, b;
                svd_round_robin(P, step, tid, &a, &b);
                const int p = min(a, b), q = max(a, b);
                const double app = re_of(G[p * (LD + 1)]), aqq = re_of(G[q * (LD + 1)]);
                const S g = G[p + q * LD];
                const double ag = sv_mod(g);
                double c = 1.0;
                S sw = s_zero<S>();
                if (app > 0.0 && aqq > 0.0 && ag > 0.0) {   // plain cyclic Jacobi: every non-zero entry is rotated
                    const double d = aqq - app;
                    const double t = (d < 0.0 ? -2.0 : 2.0) * ag / (fabs(d) + hypot(d, 2.0 * ag));
                    c = 1.0 / sqrt(1.0 + t * t);
                    sw = sv_scale(divr(g, ag), t * c);   // the phase first: t c / |g| may overflow
                }
                rc[tid] = c;
                rsw[tid] = sw;
                rpq[2 * tid] = p;
                rpq[2 * tid + 1] = q;
            }
            __syncthreads();
            // G <- R^H G R: the 2 x 2 block where rotation k's rows meet rotation l's columns
            for (int idx = tid; idx < HP * HP; idx += 256) {
                const int k = idx % HP, l = idx / HP;
                const double ck = rc[k], cl = rc[l];
                const S swk = rsw[k], swl = rsw[l];
                if (!sv_nz(swk) && !sv_nz(swl)) continue;   // neither rotates (c alone may round to 1)
                const int pk = rpq[2 * k], qk = rpq[2 * k + 1], pl = rpq[2 * l], ql = rpq[2 * l + 1];
                S b11 = G[pk + pl * LD], b12 = G[pk + ql * LD], b21 = G[qk + pl * LD], b22 = G[qk + ql * LD];
                sv_rot_cols(b11, b12, cl, swl);
                sv_rot_cols(b21, b22, cl, swl);
                sv_rot_rows(b11, b21, ck, swk);
                sv_rot_rows(b12, b22, ck, swk);
                if (k == l) {   // the rotated pair itself: real diagonal, annihilated off-diagonal
                    b11 = sv_from<S>(re_of(b11));
                    b22 = sv_from<S>(re_of(b22));
                    b12 = b21 = s_zero<S>();
                }
                G[pk + pl * LD] = b11;
                G[pk + ql * LD] = b12;
                G[qk + pl * LD] = b21;
                G[qk + ql * LD] = b22;
            }
            // J <- J R
            for (int idx = tid; idx < HP * P; idx += 256) {
                const int k = idx / P, i = idx % P;
                if (!sv_nz(rsw[k])) continue;
                const int p = rpq[2 * k], q = rpq[2 * k + 1];
                S j1 = J[i + p * LD], j2 = J[i + q * LD];
                sv_rot_cols(j1, j2, rc[k], rsw[k]);
                J[i + p * LD] = j1;
                J[i + q * LD] = j2;
            }
            __syncthreads();
        }
        off = svd_offmax<S>(G, dg, red);
        if (!(off > tol)) break;
    }
    // polish: T = 1.5 I - 0.5 J^H J into G's place, then J T to the pair's slot
    __syncthreads();
    for (int idx = tid; idx < P * P; idx += 256) {
        const int a = idx % P, c = idx / P;
        S acc = s_zero<S>();
        for (int i = 0; i < P; ++i) acc = add(acc, mul(sv_conj(J[i + a * LD]), J[i + c * LD]));
        S t = sv_scale(acc, -0.5);
        if (a == c) t = add(t, sv_from<S>(1.5));
        G[a + c * LD] = t;
    }
    __syncthreads();
    S* jo = Jout + (int64_t)pair * (P * P);
    for (int idx = tid; idx < P * P; idx += 256) {
        const int i = idx % P, c = idx / P;
        S acc = s_zero<S>();
        for (int a = 0; a < P; ++a) acc = add(acc, mul(J[i + a * LD], G[a + c * LD]));
        jo[idx] = acc;
    }
}

// ------------------------------------------------------------------ 2c. X <- X J
template <class S>
__global__ __launch_bounds__(256) void svd_apply(S* W, int m, S* V, int nv, const SvdPair* pairs, const S* Jall,
                                                 const int* pflag) {
    constexpr bool kC = std::is_same_v<S, cplx>;
    constexpr int B = SvdCfg<S>::B, P = SvdCfg<S>::P, LD = SvdCfg<S>::LD, NT = P / 16, KQ = P / 4;
    __shared__ S Js[P * LD];
    const int pair = blockIdx.y;
    if (!pflag[pair]) return;
    S* X = blockIdx.z ? V : W;
    const int rows = blockIdx.z ? nv : m;
    if ((int)blockIdx.x * kSvdApplyRows >= rows) return;
    const SvdPair pr = pairs[pair];
    const S* jp = Jall + (int64_t)pair * (P * P);
    for (int idx = threadIdx.x; idx < P * P; idx += 256) Js[(idx % P) + (idx / P) * LD] = jp[idx];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    int64_t coff[KQ];   // the columns this lane loads: local column 4 q + lk
    bool cval[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int c = svd_col(pr, 4 * q + lk, B);
        cval[q] = c >= 0;
        coff[q] = (int64_t)max(c, 0) * rows;
    }
    for (int it = 0; it < kSvdApplyRows / 64; ++it) {
        const int r0 = blockIdx.x * kSvdApplyRows + wave * (kSvdApplyRows / 4) + it * 16;
        if (r0 >= rows) break;
        const int row = r0 + li;
        const bool rv = row < rows;
        S x[KQ];
#pragma unroll
        for (int q = 0; q < KQ; ++q) x[q] = (rv && cval[q]) ? X[coff[q] + row] : s_zero<S>();
        mfma_d4 are[NT], aim[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            are[t] = aim[t] = mfma_d4{0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                // D[i][j] = sum_k J(k, 16 t + i) X(r0 + j, k)
                const S a = Js[(4 * q + lk) + (16 * t + li) * LD];
                are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(re_of(a), re_of(x[q]), are[t], 0, 0, 0);
                if constexpr (kC) {
                    are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-im_of(a), im_of(x[q]), are[t], 0, 0, 0);
                    aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(re_of(a), im_of(x[q]), aim[t], 0, 0, 0);
                    aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(im_of(a), re_of(x[q]), aim[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = svd_col(pr, 16 * t + lk + 4 * r, B);
                if (rv && c >= 0) {
                    S v;
                    set_re_im(v, are[t][r], aim[t][r]);
                    X[(int64_t)c * rows + row] = v;
                }
            }
    }
}

// ------------------------------------------------------------------ 4. finish
// out[j] = ||X(:, j)||_2, one workgroup per column
template <class S>
__global__ __launch_bounds__(256) void svd_colnorm(const S* X, int m, int64_t ld, double* out) {
    __shared__ double red[256];
    const S* x = X + (int64_t)blockIdx.x * ld;
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s += sq_abs(x[i]);
    s = sv_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrt(s);
}

// column j of Uo = W(:, perm[j]) / its norm (zero where the norm is 0), column j of Vo = V(:, perm[j])
template <class S>
__global__ __launch_bounds__(256) void svd_gather(const S* W, int m, const S* V, int n, const int* perm, const double* nrm,
                                                  S* Uo, S* Vo) {
    const int j = blockIdx.x, src = perm[j];
    if (Uo) {
        const double sg = nrm[src];
        for (int i = threadIdx.x; i < m; i += 256)
            Uo[i + (int64_t)j * m] = sg > 0.0 ? divr(W[i + (int64_t)src * m], sg) : s_zero<S>();
    }
    if (Vo)
        for (int i = threadIdx.x; i < n; i += 256) Vo[i + (int64_t)j * n] = V[i + (int64_t)src * n];
}

// coef[j] = Q(:, j)^H v
template <class S>
__global__ __launch_bounds__(256) void svd_cgs_dot(const S* Q, int m, const S* v, S* coef) {
    __shared__ double red[256];
    const S* q = Q + (int64_t)blockIdx.x * m;
    double sr = 0.0, si = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) {
        const S p = mul(sv_conj(q[i]), v[i]);
        sr += re_of(p);
        si += im_of(p);
    }
    sr = sv_block_sum(sr, red);
    si = sv_block_sum(si, red);
    if (threadIdx.x == 0) set_re_im(coef[blockIdx.x], sr, si);
}

// v -= Q coef, the columns in ascending order
template <class S>
__global__ __launch_bounds__(256) void svd_cgs_sub(const S* Q, int m, int k, const S* coef, S* v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    S acc = v[i];
    for (int j = 0; j < k; ++j) acc = sub(acc, mul(Q[i + (int64_t)j * m], coef[j]));
    v[i] = acc;
}

template <class S>
__global__ __launch_bounds__(256) void svd_unit(S* v, int m, int k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) v[i] = sv_from<S>(i == k ? 1.0 : 0.0);
}

template <class S>
__global__ __launch_bounds__(256) void svd_store_col(S* dst, const S* v, int m, const double* nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) dst[i] = divr(v[i], nrm[0]);
}

// the phase convention on column j of Z (len rows), the same phase on column j of Y (leny rows; may be null)
template <class S>
__global__ __launch_bounds__(256) void svd_phase(S* Z, int len, S* Y, int leny) {
    __shared__ double rm[256];
    __shared__ int ri[256];
    S* z = Z + (int64_t)blockIdx.x * len;
    double best = -1.0;
    int bi = 0;
    for (int i = threadIdx.x; i < len; i += 256) {
        const double a = sv_mod(z[i]);
        if (a > best) {
            best = a;
            bi = i;
        }
    }
    rm[threadIdx.x] = best;
    ri[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double o = rm[threadIdx.x + s];
            const int oi = ri[threadIdx.x + s];
            if (o > rm[threadIdx.x] || (o == rm[threadIdx.x] && oi < ri[threadIdx.x])) {
                rm[threadIdx.x] = o;
                ri[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const int k = ri[0];
    const double pm = rm[0];
    if (!(pm > 0.0)) return;
    const S p = z[k];
    const S u = divr(sv_conj(p), pm);   // a real column: exactly +-1
    __syncthreads();   // in place: every thread has its p
    for (int i = threadIdx.x; i < len; i += 256) z[i] = i == k ? sv_from<S>(pm) : mul(z[i], u);
    if (Y) {
        S* y = Y + (int64_t)blockIdx.x * leny;
        for (int i = threadIdx.x; i < leny; i += 256) y[i] = mul(y[i], u);
    }
}

}  // namespace dev

// ============================================================================ host
namespace {

constexpr int kSvdInnerSweeps = 30;   // cyclic Jacobi converges quadratically: a bound that ends the kernel, not a knob

// the pairs of one sweep, step by step (first[s] .. first[s + 1])
template <class S>
void svd_schedule(int n, std::vector<dev::SvdPair>& pairs, std::vector<int>& first) {
    constexpr int B = dev::SvdCfg<S>::B;
    const int nb = (n + B - 1) / B;
    auto width = [&](int blk) { return std::min(B, n - blk * B); };
    pairs.clear();
    first.assign(1, 0);
    if (nb == 1) {
        pairs.push_back(dev::SvdPair{0, 0, n, 0});
        first.push_back(1);
        return;
    }
    const int cnt = nb + (nb & 1);
    for (int s = 0; s < cnt - 1; ++s) {
        for (int i = 0; i < cnt / 2; ++i) {
            int a, b;
            dev::svd_round_robin(cnt, s, i, &a, &b);
            const int p = std::min(a, b), q = std::max(a, b);
            if (q >= nb) continue;   // the idle block of an odd count
            pairs.push_back(dev::SvdPair{p * B, q * B, width(p), width(q)});
        }
        first.push_back((int)pairs.size());
    }
}

// U(:, j) for the columns whose singular value is exactly 0: unit vectors in ascending order, orthogonalised
// twice against every column (the zero ones among them do nothing), accepted at norm >= thr
template <class S>
int svd_complete(hipStream_t st, S* Uo, int m, int k, const std::vector<int>& zero_cols) {
    DevBuf dv, dcoef, dnrm;
    EIGSOL_TRY(dv.alloc((size_t)m * sizeof(S)));
    EIGSOL_TRY(dcoef.alloc((size_t)k * sizeof(S)));
    EIGSOL_TRY(dnrm.alloc(sizeof(double)));
    const unsigned gm = (unsigned)((m + 255) / 256);
    size_t next = 0;
    // 0.5 holds for every matrix met so far; the lower thresholds only guarantee that the loop ends
    for (double thr = 0.5; next < zero_cols.size() && thr > 1e-3; thr *= 0.25) {
        for (int cand = 0; cand < m && next < zero_cols.size(); ++cand) {
            hipLaunchKernelGGL(dev::svd_unit<S>, dim3(gm), dim3(256), 0, st, dv.as<S>(), m, cand);
            for (int pass = 0; pass < 2; ++pass) {
                hipLaunchKernelGGL(dev::svd_cgs_dot<S>, dim3((unsigned)k), dim3(256), 0, st, Uo, m, dv.as<S>(), dcoef.as<S>());
                hipLaunchKernelGGL(dev::svd_cgs_sub<S>, dim3(gm), dim3(256), 0, st, Uo, m, k, dcoef.as<S>(), dv.as<S>());
            }
            hipLaunchKernelGGL(dev::svd_colnorm<S>, dim3(1), dim3(256), 0, st, dv.as<S>(), m, (int64_t)m, dnrm.as<double>());
            EIGSOL_HIP(hipGetLastError());
            double nrm = 0.0;
            EIGSOL_HIP(hipMemcpyAsync(&nrm, dnrm.p, sizeof(double), hipMemcpyDeviceToHost, st));
            EIGSOL_HIP(hipStreamSynchronize(st));
            if (!(nrm >= thr)) continue;
            hipLaunchKernelGGL(dev::svd_store_col<S>, dim3(gm), dim3(256), 0, st, Uo + (int64_t)zero_cols[next] * m, dv.as<S>(),
                               m, dnrm.as<double>());
            ++next;
        }
    }
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (next < zero_cols.size()) return fail(EIGSOL_E_SOLVER, "svd: could not complete the null columns of U");
    return EIGSOL_OK;
}

template <class S>
int svd_host(eigsol_ctx* ctx, int64_t m0, int64_t n0, const void* A_host, int max_sweeps, double* s_out, void* U_out,
             void* V_out, int32_t* sweeps_out, int64_t* nc_out) {
    constexpr int P = dev::SvdCfg<S>::P;
    constexpr int kDbl = std::is_same_v<S, double> ? 1 : 2;
    hipStream_t st = ctx->stream;
    const bool wide = m0 < n0;
    const int m = (int)std::max(m0, n0), n = (int)std::min(m0, n0);   // the working matrix: m x n, m >= n
    const bool anyvec = U_out || V_out;
    // the working V: the public V of a tall matrix (it also fixes U's phase), the public U of a wide one
    const bool accV = wide ? U_out != nullptr : anyvec;
    // the normalised W: the public U of a tall matrix; the public V of a wide one, which fixes both phases
    const bool needU = wide ? anyvec : U_out != nullptr;
    const int64_t cnt = (int64_t)m * n * kDbl;

    std::vector<dev::SvdPair> pairs;
    std::vector<int> first;
    svd_schedule<S>(n, pairs, first);
    const int nsteps = (int)first.size() - 1, npair = (int)pairs.size();
    int maxnp = 1;
    for (int s = 0; s < nsteps; ++s) maxnp = std::max(maxnp, first[s + 1] - first[s]);
    const int nchunk = (m + dev::kSvdGramRows - 1) / dev::kSvdGramRows;

    StageClock E, T;   // E: start, end of the sweeps, end; T: four marks per step (Gram, pair Jacobi, apply between them)
    EIGSOL_TRY(E.start(2));
    EIGSOL_TRY(T.start(4 * nsteps - 1));
    std::vector<double> tms((size_t)4 * nsteps);
    DevBuf dA, dW, dV, dpairs, dG, dJ, dpmax, dpflag, dmx;
    EIGSOL_TRY(dW.alloc((size_t)cnt * sizeof(double)));
    EIGSOL_TRY(dmx.alloc(2 * 256 * sizeof(double)));
    // ---- 0. set-up
    DevBuf& dIn = wide ? dA : dW;
    if (wide) EIGSOL_TRY(dA.alloc((size_t)cnt * sizeof(double)));
    EIGSOL_HIP(hipMemcpyAsync(dIn.p, A_host, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(E.mark(0, st));
    hipLaunchKernelGGL(dev::svd_absmax, dim3(256), dim3(256), 0, st, dIn.as<double>(), cnt, dmx.as<double>());
    EIGSOL_HIP(hipGetLastError());
    double hmx[512];
    EIGSOL_HIP(hipMemcpyAsync(hmx, dmx.p, sizeof(hmx), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    double amax = 0.0;
    for (int b = 0; b < 256; ++b) {
        if (hmx[2 * b + 1] != 0.0) return fail(EIGSOL_E_SOLVER, "svd: the matrix holds a non-finite entry");
        amax = std::max(amax, hmx[2 * b]);
    }
    const int escale = amax > 0.0 ? -std::ilogb(amax) : 0;   // 2^escale amax in [1, 2)
    // 2^escale in two exact factors: one alone overflows for entries near the smallest subnormal
    const double sc1 = std::ldexp(1.0, escale / 2), sc2 = std::ldexp(1.0, escale - escale / 2);
    if (wide) {
        hipLaunchKernelGGL(dev::svd_load_t<S>, dim3((unsigned)((n + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0, st, n, m,
                           dA.as<S>(), dW.as<S>(), 1.0);
    }
    if (escale != 0) {
        hipLaunchKernelGGL(dev::svd_scale, dim3(1024), dim3(256), 0, st, dW.as<double>(), cnt, sc1);
        hipLaunchKernelGGL(dev::svd_scale, dim3(1024), dim3(256), 0, st, dW.as<double>(), cnt, sc2);
    }
    EIGSOL_HIP(hipGetLastError());
    if (accV) {
        EIGSOL_TRY(dV.alloc((size_t)n * n * sizeof(S)));
        EIGSOL_HIP(hipMemsetAsync(dV.p, 0, (size_t)n * n * sizeof(S), st));
        hipLaunchKernelGGL(dev::svd_set_identity<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dV.as<S>(), n);
    }
    EIGSOL_TRY(dpairs.alloc((size_t)npair * sizeof(dev::SvdPair)));
    EIGSOL_HIP(hipMemcpyAsync(dpairs.p, pairs.data(), (size_t)npair * sizeof(dev::SvdPair), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(dG.alloc((size_t)maxnp * nchunk * P * P * sizeof(S)));
    EIGSOL_TRY(dJ.alloc((size_t)maxnp * P * P * sizeof(S)));
    EIGSOL_TRY(dpmax.alloc((size_t)npair * sizeof(double)));
    EIGSOL_TRY(dpflag.alloc((size_t)npair * sizeof(int)));
    constexpr size_t lds = dev::svd_jacobi_lds<S>();
    EIGSOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::svd_pair_jacobi<S>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (wide) {
        EIGSOL_HIP(hipStreamSynchronize(st));
        dA.release();
    }

    // ---- 1 .. 3. sweeps
    const double tol = std::sqrt((double)m) * DBL_EPSILON;
    std::vector<double> pmax(npair);
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    int sweeps = 0;
    int64_t above = 0;
    const unsigned ga = (unsigned)((m + dev::kSvdApplyRows - 1) / dev::kSvdApplyRows);
    for (int sweep = 1; sweep <= max_sweeps; ++sweep) {
        for (int s = 0; s < nsteps; ++s) {
            const int f = first[s], np = first[s + 1] - f;
            if (np == 0) continue;
            const dev::SvdPair* pp = dpairs.as<dev::SvdPair>() + f;
            EIGSOL_TRY(T.mark(4 * s, st));
            hipLaunchKernelGGL(dev::svd_gram<S>, dim3((unsigned)nchunk, (unsigned)np), dim3(256), 0, st, dW.as<S>(), m, pp, nchunk,
                               dG.as<S>());
            EIGSOL_TRY(T.mark(4 * s + 1, st));
            hipLaunchKernelGGL(dev::svd_pair_jacobi<S>, dim3((unsigned)np), dim3(256), lds, st, dG.as<S>(), nchunk, tol,
                               kSvdInnerSweeps, dJ.as<S>(), dpmax.as<double>() + f, dpflag.as<int>() + f);
            EIGSOL_TRY(T.mark(4 * s + 2, st));
            hipLaunchKernelGGL(dev::svd_apply<S>, dim3(ga, (unsigned)np, accV ? 2u : 1u), dim3(256), 0, st, dW.as<S>(), m,
                               dV.as<S>(), n, pp, dJ.as<S>(), dpflag.as<int>() + f);
            EIGSOL_TRY(T.mark(4 * s + 3, st));
        }
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_HIP(hipMemcpyAsync(pmax.data(), dpmax.p, (size_t)npair * sizeof(double), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        T.read(tms.data(), 4 * nsteps - 1);   // a step without pairs was not marked: zeros
        for (int s = 0; s < nsteps; ++s)
            for (int q = 0; q < 3; ++q) ms[q] += tms[4 * s + q];
        sweeps = sweep;
        above = 0;
        for (int i = 0; i < npair; ++i) {
            if (!std::isfinite(pmax[i])) return fail(EIGSOL_E_SOLVER, "svd: a non-finite Gram matrix");
            if (pmax[i] > tol) ++above;
        }
        if (above == 0) break;
    }
    EIGSOL_TRY(E.mark(1, st));

    // ---- 4. finish
    DevBuf dnrm, dperm, dUo, dVo;
    std::vector<double> nrm(n);
    EIGSOL_TRY(dnrm.alloc((size_t)n * sizeof(double)));
    hipLaunchKernelGGL(dev::svd_colnorm<S>, dim3((unsigned)n), dim3(256), 0, st, dW.as<S>(), m, (int64_t)m, dnrm.as<double>());
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipMemcpyAsync(nrm.data(), dnrm.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    std::vector<int> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return nrm[a] > nrm[b]; });
    for (int j = 0; j < n; ++j) s_out[j] = std::ldexp(nrm[perm[j]], -escale);
    if (anyvec) {
        EIGSOL_TRY(dperm.alloc((size_t)n * sizeof(int)));
        EIGSOL_HIP(hipMemcpyAsync(dperm.p, perm.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        if (needU) EIGSOL_TRY(dUo.alloc((size_t)m * n * sizeof(S)));
        if (accV) EIGSOL_TRY(dVo.alloc((size_t)n * n * sizeof(S)));
        hipLaunchKernelGGL(dev::svd_gather<S>, dim3((unsigned)n), dim3(256), 0, st, dW.as<S>(), m, dV.as<S>(), n, dperm.as<int>(),
                           dnrm.as<double>(), dUo.as<S>(), dVo.as<S>());
        EIGSOL_HIP(hipGetLastError());
        if (needU) {
            std::vector<int> zero_cols;
            for (int j = 0; j < n; ++j)
                if (nrm[perm[j]] == 0.0) zero_cols.push_back(j);
            if (!zero_cols.empty()) EIGSOL_TRY(svd_complete<S>(st, dUo.as<S>(), m, n, zero_cols));
        }
        // the public V: the working V of a tall matrix, the normalised W of a wide one
        S* zsrc = wide ? dUo.as<S>() : dVo.as<S>();
        S* zoth = wide ? dVo.as<S>() : dUo.as<S>();
        hipLaunchKernelGGL(dev::svd_phase<S>, dim3((unsigned)n), dim3(256), 0, st, zsrc, wide ? m : n, zoth, wide ? n : m);
        EIGSOL_HIP(hipGetLastError());
        void* outW = wide ? V_out : U_out;   // m x n
        void* outV = wide ? U_out : V_out;   // n x n
        if (outW) EIGSOL_HIP(hipMemcpyAsync(outW, dUo.p, (size_t)m * n * sizeof(S), hipMemcpyDeviceToHost, st));
        if (outV) EIGSOL_HIP(hipMemcpyAsync(outV, dVo.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    }
    EIGSOL_TRY(E.mark(2, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    double te[2];
    E.read(te, 2);
    ms[3] = te[1];
    for (int q = 0; q < 4; ++q) ctx->svd_ms[q] = ms[q];
    if (sweeps_out) *sweeps_out = sweeps;
    if (nc_out) *nc_out = above;
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_svd_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, const void* A_colmajor,
                     const eigsol_svd_options* opts, double* s, void* U, void* V, int32_t* sweeps,
                     int64_t* not_converged) {
    if (m < 0 || n < 0) return fail(EIGSOL_E_INVALID, "eigsol_svd_dense: negative size");
    if (m == 0 || n == 0) {
        if (sweeps) *sweeps = 0;
        if (not_converged) *not_converged = 0;
        return EIGSOL_OK;
    }
    if (!ctx || !A_colmajor || !s) return fail(EIGSOL_E_INVALID, "eigsol_svd_dense: null pointer");
    const int max_sweeps = opts ? opts->max_sweeps : 60;
    if (max_sweeps < 1) return fail(EIGSOL_E_INVALID, "eigsol_svd_dense: max_sweeps < 1");
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_svd_dense: double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, "eigsol_svd_dense: unknown dtype");
    if (std::max(m, n) > INT_MAX / 64 || m * n > (int64_t)1 << 31)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_svd_dense: more than 2^31 entries");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return dtype == EIGSOL_C128 ? svd_host<cplx>(ctx, m, n, A_colmajor, max_sweeps, s, U, V, sweeps, not_converged)
                                : svd_host<double>(ctx, m, n, A_colmajor, max_sweeps, s, U, V, sweeps, not_converged);
}

int eigsol_svd_stage_times(eigsol_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return fail(EIGSOL_E_INVALID, "eigsol_svd_stage_times: null pointer");
    for (int q = 0; q < 4; ++q) ms4[q] = ctx->svd_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
