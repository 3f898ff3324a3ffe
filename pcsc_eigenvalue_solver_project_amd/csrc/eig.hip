// Eigenvalues and right eigenvectors of a general dense matrix (gfx950; EIGSOL_F64 / EIGSOL_C128): the
// eigenvalues by the Francis sweeps on a copy of the Hessenberg matrix, every eigenvector by inverse
// iteration on the Hessenberg matrix that was kept (LAPACK xHSEIN / xLAEIN's scheme), back-transformed with
// the reduction's stored panels.  No Schur vectors are accumulated: francis.hip / zfrancis.hip are untouched.
//
//   a. the power-of-two range guard of the Francis paths (qr_range_guard, qr.hip); the eigenvalues are
//      scaled back, the vectors are computed from the scaled matrix and its eigenvalues;
//   b. H = Q^H A Q by hessenberg_blocked_vt (n >= 3; V and T of every panel kept); H is copied and
//      francis_large_* runs on the copy.  Both Francis drivers write an eigenvalue at the diagonal position
//      it deflated at, and their active window never crosses an exactly zero sub-diagonal entry, so
//      eigenvalue k belongs to the diagonal block of H that holds row k;
//   c. the host splits H where h(i+1, i) == 0 exactly; the vector of an eigenvalue of the block [kl, kr)
//      is computed on the leading kr x kr matrix and is zero below it (dhsein).  eps3 = eps ||H_block||_1
//      (safe minimum scaled where the block is null); eigenvalues of one block closer than eps3 to an
//      earlier one are moved apart by eps3 (dhsein's loop; the conjugate partner of a real matrix's
//      pair is not compared with its own pair);
//   d. eig_hsein, one workgroup per eigenvalue: the partial-pivot LU of H(0:kr, 0:kr) - lambda I, rows top
//      to bottom, the carried row in registers (column j on thread j mod NT), the next row loaded from a
//      transposed copy of H so that the load coalesces, the finished row of U stored once (packed upper
//      triangle).  A pivot below eps3 becomes eps3.  Then xLAEIN's iteration: U x = v by blocked back
//      substitution (32 rows at a time: the products with the solved part by one wave per row, the 32 x 32
//      triangle from LDS on wave 0, a power-of-two rescaling where an entry passes 2^400), accepted where
//      ||x||_1 >= 0.1 / sqrt(kr) (relative to the rescaling), else xLAEIN's next start vector, at most
//      kr - kl starts.  The start vectors are xLAEIN's on the rows of the eigenvalue's own block and zero
//      above it: the rows above then hold -U11^-1 U12 x2, the extension of the block's vector, and a
//      diagonal or null matrix gets unit vectors.  Real H with a real shift runs in real arithmetic; real H
//      with a complex shift in complex arithmetic, once per conjugate pair;
//   e. Q x by hess_backtransform (real matrices: the planes [Re | Im] as real columns), 4096 columns at a
//      time: the split of its products then does not depend on how many vectors were asked for;
//   f. unit 2-norm, the largest-modulus component (the first on ties) real positive (eig_finish); the
//      partner of a pair is written as the conjugate.
// No floating-point atomics; every sum has a fixed order that does not depend on the batch, the launch
// geometry or the selection: two calls give the same bits, and a selection the bits of the full call.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels_common.hpp"
#include "scratch.hpp"

namespace eigsol {

int francis_large_f64(eigsol_ctx* ctx, double* H, int64_t n, int maxits, double* wr, double* wi, int32_t* sweeps,
                      int32_t* fail_out);
int francis_large_c128(eigsol_ctx* ctx, cplx* H, int64_t n, int maxits, cplx* w_host, int32_t* sweeps_out,
                       int32_t* fail_out);

namespace dev {

// ------------------------------------------------------------------ scalar helpers (T = double / cplx)
__device__ __forceinline__ double eabs1(double a) { return fabs(a); }
__device__ __forceinline__ double eabs1(cplx a) { return fabs(a.re) + fabs(a.im); }
__device__ __forceinline__ double emod(double a) { return fabs(a); }
__device__ __forceinline__ double emod(cplx a) { return hypot(a.re, a.im); }
__device__ __forceinline__ double escl(double a, double s) { return a * s; }
__device__ __forceinline__ cplx escl(cplx a, double s) { return cplx{a.re * s, a.im * s}; }
__device__ __forceinline__ double ediv(double a, double b) { return a / b; }
// Smith's quotient: eps3^2 may underflow
__device__ __forceinline__ cplx ediv(cplx a, cplx b) {
    if (fabs(b.re) >= fabs(b.im)) {
        const double r = b.im / b.re, d = b.re + b.im * r;
        return cplx{(a.re + a.im * r) / d, (a.im - a.re * r) / d};
    }
    const double r = b.re / b.im, d = b.re * r + b.im;
    return cplx{(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}
template <class T> __device__ __forceinline__ T efrom(double re);
template <> __device__ __forceinline__ double efrom<double>(double re) { return re; }
template <> __device__ __forceinline__ cplx efrom<cplx>(double re) { return cplx{re, 0.0}; }
// an entry of H as the arithmetic's scalar, the shift taken off where it is diagonal
template <class T> __device__ __forceinline__ T eload(double h, bool diag, double lre, double lim);
template <> __device__ __forceinline__ double eload<double>(double h, bool diag, double lre, double) {
    return diag ? h - lre : h;
}
template <> __device__ __forceinline__ cplx eload<cplx>(double h, bool diag, double lre, double lim) {
    return diag ? cplx{h - lre, -lim} : cplx{h, 0.0};
}
template <class T> __device__ __forceinline__ T eload(cplx h, bool diag, double lre, double lim) {
    return diag ? cplx{h.re - lre, h.im - lim} : h;
}
__device__ __forceinline__ double eshfl(double v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ cplx eshfl(cplx v, int src) { return cplx{__shfl(v.re, src, 64), __shfl(v.im, src, 64)}; }
__device__ __forceinline__ double ewave_sum(double v) { return wave_sum(v); }
__device__ __forceinline__ cplx ewave_sum(cplx v) { return cplx{wave_sum(v.re), wave_sum(v.im)}; }

// ------------------------------------------------------------------ preparation
// Ht(j, i) = H(i, j) on and above the sub-diagonal, 0 below it: row i of H is n contiguous scalars
template <class S>
__global__ __launch_bounds__(256) void eig_transpose(const S* H, int n, S* Ht) {
    __shared__ S tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {   // column j0 + r of H, rows i0 + tx
        const int i = i0 + tx, j = j0 + r;
        S v = s_zero<S>();
        if (i < n && j < n && j + 1 >= i) v = H[i + (int64_t)j * n];
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {   // row i0 + r of H, columns j0 + tx
        const int i = i0 + r, j = j0 + tx;
        if (i < n && j < n) Ht[(int64_t)i * n + j] = tile[tx][r];
    }
}

template <class S>
__global__ __launch_bounds__(256) void eig_subdiag(const S* H, int n, S* sub) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i + 1 < n) sub[i] = H[(i + 1) + (int64_t)i * n];
}

// out[j] = sum of |H(i, j)| over the rows of column j's diagonal block on and above the sub-diagonal
// (kl[j]: the block's first row; the entry below the block's last row is the zero that ends it): one wave
// per column, lanes stride the rows, then the butterfly
template <class S>
__global__ __launch_bounds__(256) void eig_colsum(const S* H, int n, const int* kl, double* out) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;
    const int last = min(j + 1, n - 1);
    double s = 0.0;
    for (int i = kl[j] + lane; i <= last; i += 64) s += emod(H[i + (int64_t)j * n]);
    s = wave_sum(s);
    if (lane == 0) out[j] = s;
}

// ------------------------------------------------------------------ inverse iteration
// One eigenvalue: the (perturbed) shift, eps3 of its block, the block's rows [kl, kr), and where the vector
// goes: column col (and, for a complex shift of a real matrix, column colim of the imaginary plane).
struct EigJob {
    double lre, lim, eps3;
    int kl, kr, col, colim;
};
struct EigOut {
    double* re;   // real H: plane of real parts, leading dimension n
    double* im;   // real H, complex shift: plane of imaginary parts
    cplx* z;      // complex H
};

constexpr int kEigBlock = 32;          // rows of back substitution solved together
constexpr double kEigBig = 0x1p400;    // an entry of x above it rescales x by kEigDown
constexpr double kEigDown = 0x1p-500;

__device__ __forceinline__ int64_t urow(int i, int kr) {   // start of row i in the packed upper triangle
    return (int64_t)i * kr - ((int64_t)i * (i - 1)) / 2;
}

__device__ __forceinline__ void eout(const EigOut& o, const EigJob& jb, int n, int i, double v) {
    o.re[(int64_t)jb.col * n + i] = v;
}
template <class HS>
__device__ __forceinline__ void eout(const EigOut& o, const EigJob& jb, int n, int i, cplx v) {
    if constexpr (std::is_same_v<HS, cplx>) {
        o.z[(int64_t)jb.col * n + i] = v;
    } else {
        o.re[(int64_t)jb.col * n + i] = v.re;
        o.im[(int64_t)jb.colim * n + i] = v.im;
    }
}

// HS: H's scalar; T: the arithmetic's.  NT threads, EPT columns per thread (kr <= NT EPT).  U: ustride
// scalars per resident job, xw: n scalars per resident job.  kPre: the row after next is loaded a step
// ahead (held in registers; off where three rows of registers spill: launch_hsein_cfg).
template <class HS, class T, int NT, int EPT, bool kPre>
__global__ __launch_bounds__(NT) void eig_hsein(int n, const HS* __restrict__ Ht, const EigJob* __restrict__ jobs,
                                                T* Uall, int64_t ustride, T* xall, EigOut out, int* nfail) {
    constexpr int BS = kEigBlock, NW = NT / 64;
    __shared__ T s_pe[2][2];
    __shared__ T s_blk[BS][BS + 1];
    __shared__ T s_rhs[BS];
    __shared__ double s_ctl[2];
    const EigJob jb = jobs[blockIdx.x];
    const int kr = jb.kr, kl = jb.kl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T* const U = Uall + (int64_t)blockIdx.x * ustride;
    T* const x = xall + (int64_t)blockIdx.x * n;
    const double eps3 = jb.eps3;
    const T zero = efrom<T>(0.0);

    // ---- the factorisation: row i of U is final once row i + 1 has been eliminated against it
    auto load_row = [&](int i, T (&dst)[EPT]) {
        const HS* hr = Ht + (int64_t)i * n;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * NT;
            dst[e] = (j < kr && j + 1 >= i) ? eload<T>(hr[j], j == i, jb.lre, jb.lim) : zero;
        }
    };
    T row[EPT], nxt[EPT], pre[EPT];
    load_row(0, row);
    if (kr > 1) load_row(1, nxt);
    for (int i = 0; i + 1 < kr; ++i) {
        if (kPre && i + 2 < kr) load_row(i + 2, pre);
        if (tid == i % NT) {
            const int ei = i / NT;
#pragma unroll
            for (int e = 0; e < EPT; ++e)
                if (e == ei) {
                    s_pe[i & 1][0] = row[e];
                    s_pe[i & 1][1] = nxt[e];
                }
        }
        __syncthreads();
        T piv = s_pe[i & 1][0];
        const T sd = s_pe[i & 1][1];
        if (eabs1(piv) < eabs1(sd)) {   // interchange rows i and i + 1
            const T mult = ediv(piv, sd);
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int j = tid + e * NT;
                if (j > i) {
                    const T t = nxt[e];
                    nxt[e] = sub(row[e], mul(mult, t));
                    row[e] = t;
                } else if (j == i) {
                    row[e] = sd;
                    nxt[e] = zero;
                }
            }
        } else {
            if (eabs1(piv) < eps3) piv = efrom<T>(eps3);
            const T mult = ediv(sd, piv);
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int j = tid + e * NT;
                if (j > i) {
                    nxt[e] = sub(nxt[e], mul(mult, row[e]));
                } else if (j == i) {
                    row[e] = piv;
                    nxt[e] = zero;
                }
            }
        }
        T* const ur = U + urow(i, kr) - i;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * NT;
            if (j >= i && j < kr) ur[j] = row[e];
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) row[e] = nxt[e];
        if (kPre) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) nxt[e] = pre[e];
        } else if (i + 2 < kr) {
            load_row(i + 2, nxt);
        }
    }
    {   // the last row: its pivot
        T* const ur = U + urow(kr - 1, kr) - (kr - 1);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * NT;
            if (j == kr - 1) ur[j] = eabs1(row[e]) < eps3 ? efrom<T>(eps3) : row[e];
        }
    }
    __syncthreads();

    // ---- xLAEIN's iteration on U
    const double rootn = sqrt((double)kr);
    const double growto = 0.1 / rootn;
    const double rtemp = eps3 / (rootn + 1.0);
    const int maxits = kr - kl;
    bool accepted = false;
    for (int its = 1; its <= maxits && !accepted; ++its) {
        double scale = 1.0;   // x solves U x = scale v
        auto start = [&](int i) -> double {
            if (i < kl) return 0.0;
            if (its == 1) return eps3;
            double v = i == kl ? eps3 : rtemp;
            if (i == kr - its + 1) v -= eps3 * rootn;
            return v;
        };
        for (int i0 = (kr - 1) / BS * BS; i0 >= 0; i0 -= BS) {
            const int i1 = min(kr, i0 + BS), bs = i1 - i0;
            // the block's right-hand sides less the products with the solved part: one wave per row
            for (int r = wave; r < bs; r += NW) {
                const int i = i0 + r;
                const T* const ur = U + urow(i, kr) - i;
                T acc = zero;
                for (int j = i1 + lane; j < kr; j += 64) acc = add(acc, mul(ur[j], x[j]));
                acc = ewave_sum(acc);
                if (lane == 0) s_rhs[r] = sub(efrom<T>(scale * start(i)), acc);
            }
            for (int idx = tid; idx < bs * bs; idx += NT) {
                const int r = idx / bs, c = idx % bs;
                if (c >= r) s_blk[r][c] = U[urow(i0 + r, kr) + (c - r)];
            }
            __syncthreads();
            if (wave == 0) {   // the triangle, last column first; lane r keeps row r's right-hand side and x
                T rhs = lane < bs ? s_rhs[lane] : zero;
                T xl = zero;
                double pend = 1.0;
                for (int c = bs - 1; c >= 0; --c) {
                    T xc = ediv(eshfl(rhs, c), s_blk[c][c]);
                    if (eabs1(xc) > kEigBig) {
                        xc = escl(xc, kEigDown);
                        rhs = escl(rhs, kEigDown);
                        xl = escl(xl, kEigDown);
                        pend *= kEigDown;
                    }
                    if (lane == c) xl = xc;
                    if (lane < c) rhs = sub(rhs, mul(s_blk[lane][c], xc));
                }
                if (lane < bs) x[i0 + lane] = xl;
                if (lane == 0) s_ctl[0] = pend;
            }
            __syncthreads();
            const double pend = s_ctl[0];
            if (pend != 1.0) {   // (the same on every thread)
                for (int j = i1 + tid; j < kr; j += NT) x[j] = escl(x[j], pend);
                scale *= pend;
                __syncthreads();
            }
        }
        if (wave == 0) {
            double s = 0.0;
            for (int j = lane; j < kr; j += 64) s += eabs1(x[j]);
            s = wave_sum(s);
            if (lane == 0) s_ctl[1] = s;
        }
        __syncthreads();
        accepted = s_ctl[1] >= growto * scale;
        __syncthreads();
    }
    if (!accepted && tid == 0) atomicAdd(nfail, 1);

    // ---- largest |re| + |im| -> 1 (xLAEIN's normalisation); zero below the block
    if (wave == 0) {
        double m = 0.0;
        for (int j = lane; j < kr; j += 64) m = fmax(m, eabs1(x[j]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
        if (lane == 0) s_ctl[0] = m;
    }
    __syncthreads();
    const double mx = s_ctl[0];
    const double inv = mx > 0.0 && mx <= DBL_MAX ? 1.0 / mx : 1.0;
    for (int i = tid; i < n; i += NT) {
        const T v = i < kr ? escl(x[i], inv) : zero;
        if constexpr (std::is_same_v<T, double>) eout(out, jb, n, i, v);
        else eout<HS>(out, jb, n, i, v);
    }
}

// ------------------------------------------------------------------ normalisation
// One vector: column col (real matrices: of the real plane, colim of the imaginary one, -1 for a real
// eigenvalue) -> column out1 of V and, conjugated, column out2 (-1: none, either).
struct EigFin {
    int col, colim, out1, out2;
};

// unit 2-norm, the largest-modulus component (the first on ties) real positive; one workgroup per vector,
// sums by thread stride, wave butterfly, then wave order
template <bool kPlanar>
__global__ __launch_bounds__(256) void eig_finish(int n, const double* W, const EigFin* fins, cplx* V) {
    __shared__ double sv[256];
    __shared__ int si[256];
    __shared__ double sw[4];
    const EigFin f = fins[blockIdx.x];
    auto get = [&](int i) -> cplx {
        if constexpr (kPlanar)
            return cplx{W[(int64_t)f.col * n + i], f.colim >= 0 ? W[(int64_t)f.colim * n + i] : 0.0};
        else
            return V[(int64_t)f.col * n + i];
    };
    double bv = -1.0, s2 = 0.0;
    int bi = INT_MAX;
    for (int i = threadIdx.x; i < n; i += 256) {
        const cplx z = get(i);
        const double v = hypot(z.re, z.im);
        s2 += z.re * z.re + z.im * z.im;
        if (v > bv) { bv = v; bi = i; }
    }
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s2;
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
    const double nrm = sqrt(((sw[0] + sw[1]) + sw[2]) + sw[3]);
    const bool ok = k < n && pm > 0.0 && nrm > 0.0;
    const cplx p = ok ? get(k) : cplx{1.0, 0.0};
    const double inv = ok ? 1.0 / nrm : 1.0;
    const cplx u = ok ? cplx{p.re / pm, -p.im / pm} : cplx{1.0, 0.0};
    __syncthreads();   // in place where V is read: every thread has its p
    for (int i = threadIdx.x; i < n; i += 256) {
        cplx z = get(i);
        if (kPlanar && f.colim < 0) z = cplx{p.re < 0.0 ? -z.re : z.re, 0.0};
        else z = (ok && i == k) ? cplx{pm, 0.0} : mul(z, u);
        z = cplx{z.re * inv, z.im * inv};
        if (f.out1 >= 0) V[(int64_t)f.out1 * n + i] = z;
        if (f.out2 >= 0) V[(int64_t)f.out2 * n + i] = cplx{z.re, -z.im};
    }
}

}  // namespace dev

// ============================================================================ host
namespace {

// The workspace of the resident eigenvalues (U and x) stays below this: a 4096^2 real matrix's complex
// shifts take 128 MiB of U each, so 32 GiB keeps 256 workgroups, one per CU, resident; half of the free
// device memory where that is less.
constexpr size_t kEigWorkCap = (size_t)32 << 30;

template <class HS, class T, int NT, int EPT>
void launch_hsein_cfg(hipStream_t st, int nblocks, int n, const HS* Ht, const dev::EigJob* jobs, T* U, int64_t ustride,
                      T* xw, dev::EigOut out, int* nfail) {
    // complex rows of 8 and 16 columns per thread spill with a third row in registers (measured: 6 x slower at 4500)
    constexpr bool kPre = std::is_same_v<T, double> || EPT <= 4;
    hipLaunchKernelGGL((dev::eig_hsein<HS, T, NT, EPT, kPre>), dim3(nblocks), dim3(NT), 0, st, n, Ht, jobs, U, ustride,
                       xw, out, nfail);
}

// the smallest geometry that holds maxkr columns: 256 threads up to 1024 columns, 1024 threads above
template <class HS, class T>
void launch_hsein(hipStream_t st, int nblocks, int maxkr, int n, const HS* Ht, const dev::EigJob* jobs, T* U,
                  int64_t ustride, T* xw, dev::EigOut out, int* nfail) {
    if (maxkr <= 256) launch_hsein_cfg<HS, T, 256, 1>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
    else if (maxkr <= 512) launch_hsein_cfg<HS, T, 256, 2>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
    else if (maxkr <= 1024) launch_hsein_cfg<HS, T, 256, 4>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
    else if (maxkr <= 2048) launch_hsein_cfg<HS, T, 1024, 2>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
    else if (maxkr <= 4096) launch_hsein_cfg<HS, T, 1024, 4>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
    else if (maxkr <= 8192) launch_hsein_cfg<HS, T, 1024, 8>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
    else launch_hsein_cfg<HS, T, 1024, 16>(st, nblocks, n, Ht, jobs, U, ustride, xw, out, nfail);
}

// every job of one arithmetic, `batch` of them resident at a time (0: as many as kEigWorkCap holds)
template <class HS, class T>
int run_jobs(hipStream_t st, int n, const HS* Ht, const std::vector<dev::EigJob>& jobs, int batch, dev::EigOut out,
             int* dfail, DevBuf& djobs, DevBuf& dU, DevBuf& dx) {
    if (jobs.empty()) return EIGSOL_OK;
    int maxkr = 1;
    for (const auto& j : jobs) maxkr = std::max(maxkr, j.kr);
    const int64_t ustride = (int64_t)maxkr * (maxkr + 1) / 2;
    const size_t per = ((size_t)ustride + (size_t)n) * sizeof(T);
    int64_t B = batch;
    if (B <= 0) {
        size_t cap = kEigWorkCap, freeb = 0, totalb = 0;
        if (hipMemGetInfo(&freeb, &totalb) == hipSuccess) cap = std::min(cap, freeb / 2);
        B = std::max<int64_t>(1, (int64_t)(cap / per));
    }
    B = std::min<int64_t>(B, (int64_t)jobs.size());
    EIGSOL_TRY(djobs.alloc(jobs.size() * sizeof(dev::EigJob)));
    EIGSOL_TRY(dU.alloc((size_t)B * ustride * sizeof(T)));
    EIGSOL_TRY(dx.alloc((size_t)B * n * sizeof(T)));
    EIGSOL_HIP(hipMemcpyAsync(djobs.p, jobs.data(), jobs.size() * sizeof(dev::EigJob), hipMemcpyHostToDevice, st));
    for (int64_t q0 = 0; q0 < (int64_t)jobs.size(); q0 += B) {
        const int nb = (int)std::min<int64_t>(B, (int64_t)jobs.size() - q0);
        int mk = 1;
        for (int q = 0; q < nb; ++q) mk = std::max(mk, jobs[q0 + q].kr);
        launch_hsein<HS, T>(st, nb, mk, n, Ht, djobs.as<dev::EigJob>() + q0, dU.as<T>(), ustride, dx.as<T>(), out, dfail);
    }
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

inline bool is_zero_h(double a) { return a == 0.0; }
inline bool is_zero_h(cplx a) { return a.re == 0.0 && a.im == 0.0; }
inline bool is_finite_h(double a) { return std::isfinite(a); }
inline bool is_finite_h(cplx a) { return std::isfinite(a.re) && std::isfinite(a.im); }

template <class S> struct EigOps;
template <> struct EigOps<double> {
    static int reduce(hipStream_t st, double* A, int64_t n, double* V, double* T) { return hessenberg_blocked_vt_f64(st, A, n, V, T); }
    static int nb() { return hess_panel_width_f64(); }
};
template <> struct EigOps<cplx> {
    static int reduce(hipStream_t st, cplx* A, int64_t n, cplx* V, cplx* T) { return hessenberg_blocked_vt_c128(st, A, n, V, T); }
    static int nb() { return hess_panel_width_c128(); }
};

constexpr int64_t kBackChunk = 4096;   // columns per back-transformation: see step e above

template <class S>
int eig_host(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, int batch, int64_t nsel, const int64_t* sel,
             double* w_out, void* V_out, int64_t* m_out, int32_t* iterations, int32_t* converged,
             int64_t* not_converged) {
    constexpr bool kReal = std::is_same_v<S, double>;
    using Ops = EigOps<S>;
    hipStream_t st = ctx->stream;
    const int NB = Ops::nb();
    const int64_t npan = n >= 3 ? (n - 2 + NB - 1) / NB : 0;
    StageClock clock;
    EIGSOL_TRY(clock.start(4));
    DevBuf dH, dH2, dV, dT;
    EIGSOL_TRY(dH.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dH2.alloc((size_t)n * n * sizeof(S)));
    if (V_out && npan) {
        EIGSOL_TRY(dV.alloc((size_t)npan * n * NB * sizeof(S)));
        EIGSOL_TRY(dT.alloc((size_t)npan * NB * NB * sizeof(S)));
    }
    EIGSOL_HIP(hipMemcpyAsync(dH.p, A_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(clock.mark(0, st));
    // ---- a. range guard; b. reduction with the panels kept, Francis on a copy
    int escale = 0;
    EIGSOL_TRY(qr_range_guard(st, dH.as<double>(), (kReal ? 1 : 2) * n * n, &escale));
    if (n >= 3) EIGSOL_TRY(Ops::reduce(st, dH.as<S>(), n, dV.as<S>(), dT.as<S>()));
    EIGSOL_HIP(hipMemcpyAsync(dH2.p, dH.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToDevice, st));
    EIGSOL_TRY(clock.mark(1, st));
    std::vector<double> wr(n), wi(n, 0.0);   // of the (scaled) matrix the vectors are computed from
    int32_t sweeps = 0, failed = 0;
    if constexpr (kReal) {
        EIGSOL_TRY(francis_large_f64(ctx, dH2.as<double>(), n, max_iter, wr.data(), wi.data(), &sweeps, &failed));
    } else {
        std::vector<cplx> wc(n);
        EIGSOL_TRY(francis_large_c128(ctx, dH2.as<cplx>(), n, max_iter, wc.data(), &sweeps, &failed));
        for (int64_t i = 0; i < n; ++i) { wr[i] = wc[i].re; wi[i] = wc[i].im; }
    }
    dH2.release();
    EIGSOL_TRY(clock.mark(2, st));
    for (int64_t i = 0; i < n; ++i) {
        w_out[2 * i] = escale ? std::ldexp(wr[i], -escale) : wr[i];
        w_out[2 * i + 1] = escale ? std::ldexp(wi[i], -escale) : wi[i];
    }
    if (iterations) *iterations = sweeps;
    if (converged) *converged = failed ? 0 : 1;
    if (not_converged) *not_converged = 0;
    const int64_t m = V_out ? (sel ? nsel : n) : 0;
    *m_out = m;
    if (m == 0) {
        EIGSOL_HIP(hipStreamSynchronize(st));
        clock.read(ctx->eig_ms, 4);   // the two stages marked so far
        return EIGSOL_OK;
    }
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(wr[i]) || !std::isfinite(wi[i]))
            return fail(EIGSOL_E_SOLVER, "eig: a non-finite eigenvalue (does the matrix hold a non-finite entry?)");

    // ---- c. the plan: blocks, eps3, perturbation, jobs
    DevBuf dsub, dHt, dkl, dcs;
    std::vector<S> subd(std::max<int64_t>(n, 1));
    if (n > 1) {
        EIGSOL_TRY(dsub.alloc((size_t)n * sizeof(S)));
        hipLaunchKernelGGL(dev::eig_subdiag<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dH.as<S>(), (int)n,
                           dsub.as<S>());
        EIGSOL_HIP(hipMemcpyAsync(subd.data(), dsub.p, (size_t)(n - 1) * sizeof(S), hipMemcpyDeviceToHost, st));
    }
    EIGSOL_TRY(dHt.alloc((size_t)n * n * sizeof(S)));
    {
        const unsigned g = (unsigned)((n + 31) / 32);
        hipLaunchKernelGGL(dev::eig_transpose<S>, dim3(g, g), dim3(256), 0, st, dH.as<S>(), (int)n, dHt.as<S>());
    }
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipStreamSynchronize(st));
    std::vector<int> kl_of(n), kr_of(n);
    {
        int kl = 0;
        for (int64_t i = 0; i < n; ++i) {
            kl_of[i] = kl;
            if (i + 1 == n || is_zero_h(subd[i])) {
                for (int64_t q = kl; q <= i; ++q) kr_of[q] = (int)i + 1;
                kl = (int)i + 1;
            } else if (!is_finite_h(subd[i])) {
                return fail(EIGSOL_E_SOLVER, "eig: the Hessenberg matrix holds a non-finite entry");
            }
        }
    }
    std::vector<double> colsum(n);
    EIGSOL_TRY(dkl.alloc((size_t)n * sizeof(int)));
    EIGSOL_TRY(dcs.alloc((size_t)n * sizeof(double)));
    EIGSOL_HIP(hipMemcpyAsync(dkl.p, kl_of.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dev::eig_colsum<S>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, dH.as<S>(), (int)n, dkl.as<int>(),
                       dcs.as<double>());
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipMemcpyAsync(colsum.data(), dcs.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    dH.release();   // only the transposed copy is read from here on
    // conjugate pairs of a real matrix: neighbours with equal real parts and opposite imaginary parts
    std::vector<int> partner(n, -1);
    if constexpr (kReal) {
        for (int64_t i = 0; i + 1 < n; ++i)
            if (partner[i] < 0 && wi[i] != 0.0 && wr[i + 1] == wr[i] && wi[i + 1] == -wi[i] && kr_of[i] == kr_of[i + 1]) {
                partner[i] = (int)i + 1;
                partner[i + 1] = (int)i;
            }
    }
    std::vector<double> eps3(n), pr(n), pi(n);
    for (int64_t b0 = 0; b0 < n; b0 = kr_of[b0]) {
        const int64_t b1 = kr_of[b0];
        double hnorm = 0.0;
        for (int64_t j = b0; j < b1; ++j) hnorm = std::max(hnorm, colsum[j]);
        if (!std::isfinite(hnorm)) return fail(EIGSOL_E_SOLVER, "eig: the Hessenberg matrix holds a non-finite entry");
        const double e3 = hnorm > 0.0 ? hnorm * DBL_EPSILON : DBL_MIN * ((double)(b1 - b0) / DBL_EPSILON);
        for (int64_t k = b0; k < b1; ++k) {
            eps3[k] = e3;
            if (partner[k] >= 0 && partner[k] < k) {   // the pair's second: the conjugate of its first
                pr[k] = pr[k - 1];
                pi[k] = -pi[k - 1];
                continue;
            }
            double xr = wr[k], xi = wi[k];
            for (int64_t guard = 0; guard <= k - b0; ++guard) {   // dhsein: away from every earlier one
                bool moved = false;
                for (int64_t i = k - 1; i >= b0; --i)
                    if (std::fabs(pr[i] - xr) + std::fabs(pi[i] - xi) < e3) {
                        xr += e3;
                        moved = true;
                        break;
                    }
                if (!moved) break;
            }
            pr[k] = xr;
            pi[k] = xi;
        }
    }
    // jobs: one per selected eigenvalue; one per conjugate pair of a real matrix (on the member with Im > 0)
    std::vector<dev::EigJob> jobs_r, jobs_c;
    std::vector<dev::EigFin> fins;
    std::vector<int> job_of(n, -1);   // real matrices: the entry of fins that serves eigenvalue k
    int ncol = 0, ncolc = 0;           // real matrices: columns of the real plane / of the imaginary one
    for (int64_t j = 0; j < m; ++j) {
        const int64_t k = sel ? sel[j] : j;
        if constexpr (!kReal) {
            jobs_c.push_back(dev::EigJob{pr[k], pi[k], eps3[k], kl_of[k], kr_of[k], (int)j, -1});
            fins.push_back(dev::EigFin{(int)j, -1, (int)j, -1});
        } else {
            int64_t prim = k;
            if (partner[k] >= 0 && wi[k] < 0.0) prim = partner[k];
            if (job_of[prim] < 0) {
                job_of[prim] = (int)fins.size();
                const bool cx = wi[prim] != 0.0;
                dev::EigJob jb{pr[prim], pi[prim], eps3[prim], kl_of[prim], kr_of[prim], ncol++, cx ? ncolc++ : -1};
                (cx ? jobs_c : jobs_r).push_back(jb);
                fins.push_back(dev::EigFin{jb.col, jb.colim, -1, -1});
            }
            const int fi = job_of[prim];
            const bool cj = prim != k;   // this eigenvalue takes the conjugate of the job's vector
            if (!cj && fins[fi].out1 < 0) fins[fi].out1 = (int)j;
            else if (cj && fins[fi].out2 < 0) fins[fi].out2 = (int)j;
            else fins.push_back(dev::EigFin{fins[fi].col, fins[fi].colim, cj ? -1 : (int)j, cj ? (int)j : -1});   // repeated
        }
    }
    // ---- d. inverse iteration
    DevBuf dW, dZ, dfail, djr, djc, dUr, dUc, dxr, dxc, dfin;
    EIGSOL_TRY(dfail.alloc(64));
    EIGSOL_HIP(hipMemsetAsync(dfail.p, 0, 64, st));
    EIGSOL_TRY(dZ.alloc((size_t)n * m * sizeof(cplx)));
    int64_t wcols = 0;
    if constexpr (kReal) {
        wcols = (int64_t)ncol + ncolc;
        EIGSOL_TRY(dW.alloc((size_t)n * wcols * sizeof(double)));
        for (auto& f : fins)
            if (f.colim >= 0) f.colim += ncol;
        dev::EigOut out{dW.as<double>(), dW.as<double>() + (size_t)n * ncol, nullptr};
        EIGSOL_TRY((run_jobs<double, double>(st, (int)n, dHt.as<double>(), jobs_r, batch, out, dfail.as<int>(), djr, dUr, dxr)));
        EIGSOL_TRY((run_jobs<double, cplx>(st, (int)n, dHt.as<double>(), jobs_c, batch, out, dfail.as<int>(), djc, dUc, dxc)));
    } else {
        dev::EigOut out{nullptr, nullptr, dZ.as<cplx>()};
        EIGSOL_TRY((run_jobs<cplx, cplx>(st, (int)n, dHt.as<cplx>(), jobs_c, batch, out, dfail.as<int>(), djc, dUc, dxc)));
    }
    int nfail = 0;
    EIGSOL_HIP(hipMemcpyAsync(&nfail, dfail.p, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(3, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    for (DevBuf* b : {&dUr, &dUc, &dxr, &dxc, &dHt}) b->release();

    // ---- e. back-transformation, f. normalisation
    if constexpr (kReal) {
        if (npan)
            for (int64_t c0 = 0; c0 < wcols; c0 += kBackChunk)
                EIGSOL_TRY(hess_backtransform_f64(st, n, std::min(kBackChunk, wcols - c0), dV.as<double>(), dT.as<double>(),
                                                  dW.as<double>() + (size_t)c0 * n, n));
    } else if (npan) {
        for (int64_t c0 = 0; c0 < m; c0 += kBackChunk)
            EIGSOL_TRY(hess_backtransform_c128(st, n, std::min(kBackChunk, m - c0), dV.as<cplx>(), dT.as<cplx>(),
                                               dZ.as<cplx>() + (size_t)c0 * n, n));
    }
    EIGSOL_TRY(dfin.alloc(fins.size() * sizeof(dev::EigFin)));
    EIGSOL_HIP(hipMemcpyAsync(dfin.p, fins.data(), fins.size() * sizeof(dev::EigFin), hipMemcpyHostToDevice, st));
    if constexpr (kReal)
        hipLaunchKernelGGL(dev::eig_finish<true>, dim3((unsigned)fins.size()), dim3(256), 0, st, (int)n, dW.as<double>(),
                           dfin.as<dev::EigFin>(), dZ.as<cplx>());
    else
        hipLaunchKernelGGL(dev::eig_finish<false>, dim3((unsigned)fins.size()), dim3(256), 0, st, (int)n, nullptr,
                           dfin.as<dev::EigFin>(), dZ.as<cplx>());
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipMemcpyAsync(V_out, dZ.p, (size_t)n * m * sizeof(cplx), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(4, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (not_converged) *not_converged = nfail;
    clock.read(ctx->eig_ms, 4);
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_eig_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_eig_options* opts,
                     double* w, void* V, int64_t* m_out, int32_t* iterations, int32_t* converged,
                     int64_t* not_converged) {
    if (n < 0) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: negative order");
    if (n == 0) {
        if (m_out) *m_out = 0;
        if (iterations) *iterations = 0;
        if (converged) *converged = 1;
        if (not_converged) *not_converged = 0;
        return EIGSOL_OK;
    }
    if (!ctx || !A_colmajor || !w || !m_out) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: null pointer");
    const int max_iter = opts ? opts->max_iterations : 1000;
    const int batch = opts ? opts->batch : 0;
    const int64_t* sel = opts ? opts->sel : nullptr;
    const int64_t nsel = sel ? opts->nsel : 0;
    if (max_iter < 1 || batch < 0) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: max_iterations < 1 or batch < 0");
    if (opts && !opts->sel && opts->nsel != 0) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: nsel without sel");
    if (sel) {
        if (nsel < 0 || nsel > INT_MAX / 2) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: bad selection count");
        for (int64_t j = 0; j < nsel; ++j)
            if (sel[j] < 0 || sel[j] >= n) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: a selected index outside 0 .. n-1");
    }
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_eig_dense: double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, "eigsol_eig_dense: unknown dtype");
    if (n > (dtype == EIGSOL_C128 ? hess_max_order_c128() : hess_max_order_f64()))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_eig_dense: n above the order the blocked Hessenberg reduction accepts");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return dtype == EIGSOL_C128
               ? eig_host<cplx>(ctx, n, A_colmajor, max_iter, batch, nsel, sel, w, V, m_out, iterations, converged, not_converged)
               : eig_host<double>(ctx, n, A_colmajor, max_iter, batch, nsel, sel, w, V, m_out, iterations, converged,
                                  not_converged);
}

int eigsol_eig_stage_times(eigsol_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return fail(EIGSOL_E_INVALID, "eigsol_eig_stage_times: null pointer");
    for (int q = 0; q < 4; ++q) ms4[q] = ctx->eig_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
