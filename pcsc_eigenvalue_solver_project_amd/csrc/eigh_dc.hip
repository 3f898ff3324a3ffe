// Divide and conquer for the symmetric tridiagonal eigenproblem (gfx950): Cuppen's method with Gu and
// Eisenstat's stabilisation (LAPACK dstedc / dlaed1-4's scheme), the tridiagonal stage of eigh under
// EIGSOL_EIGH_METHOD_DC.  T = (d, e) is real with e > 0 inside a split block.
//
//   scale (host)  every split block times the power of two that brings its largest entry into [1, 2) (exact, undone
//                 on the eigenvalues): dlaed2's tolerance assumes poles of order 1, as dstedc's own scaling provides.
//   plan (host)   every split block is halved down to leaves of order <= L (64; EIGSOL_DC_LEAF); at a cut c
//                 rho = e_c, d_c -= rho, d_{c+1} -= rho, so T = diag(T_1', T_2') + rho v v^T, v = e_c + e_{c+1}.
//                 A node's level is its height above its deepest leaf; a level's merges run together.
//   leaves        dc_leaf: one wave per leaf, implicit-shift QL.  d and e live in the wave's registers (lane t
//                 holds entry t, a step reads them by v_readlane), every lane computes the same rotation
//                 scalars and owns one row of the vector matrix, kept in LDS.
//   per level     dc_gather_z: z = (last row of Q_1, first row of Q_2) of every merge; one copy of the
//                 values and z to the host; dc_deflate_host (dlaed2's rules; eigsol_dc_deflate is the same
//                 function); dc_rotate applies the recorded rotations to the columns of Q (a thread owns a
//                 row and walks the merge's list in order); dc_permute writes the columns, kept ones first,
//                 into the second matrix; dc_secular: one lane per root, the root relative to its nearer
//                 pole (origin chosen by the sign of f at the midpoint) by bisection on mu, poles and z^2
//                 staged through LDS and read as broadcasts; dc_loewner: zhat_j from the running product of
//                 ratios, every difference formed as (d_o - d_j) + mu; dc_vectors: u_ji = zhat_j /
//                 ((d_j - d_o) - mu_i), unit columns, into the third matrix; one GEMM per merge on the fp64
//                 matrix cores (hess_gemm_nn_f64) back into Q; dc_copy_deflated for the other columns.
// A merge leaves its kept roots first (ascending) and the deflated values after them; the next level's
// deflation sorts the poles, and the caller sorts all values once at the top.
// No floating-point atomics; every sum and product has a fixed order, so two runs give the same bits.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "cholesky.hpp"
#include "kernels_common.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

constexpr int kDcLeafMax = 64;        // a leaf is one wave: lane t holds d_t, e_t and row t of the vectors
constexpr int kDcLeafSweeps = 60;     // QL sweeps per eigenvalue before it is counted as not converged
constexpr int kDcChunk = 1024;        // poles staged through LDS at a time
constexpr int kDcSecularCap = 400;    // bisection steps per root

struct DcLeaf {
    int b0, bn;
};
// one merge of a level: columns / rows [lo, lo + n) of Q, k kept poles, its rotations rot[rot0 .. rot0 + nrot)
struct DcMerge {
    int lo, n, k, rot0, nrot, pad;
    double rho;
};
struct DcRot {
    int a, b;   // global columns: (a, b) <- (c a + s b, c b - s a)
    double c, s;
};

__device__ __forceinline__ double dc_lane(double v, int t) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), t);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), t);
    return __hiloint2double(hi, lo);
}

// Implicit-shift QL (EISPACK tql2's recurrence) on the leaf's tridiagonal.  Qs[c * 64 + lane] is entry
// (lane, c) of the vector matrix: a lane touches its own row only.  Q(b0 + r, b0 + c) and lam[b0 + c] out.
__global__ __launch_bounds__(64) void dc_leaf(int n, const double* d, const double* e, const DcLeaf* leaves, double* Q,
                                              double* lam, int* ncap) {
    __shared__ double Qs[kDcLeafMax * 64];
    const DcLeaf lf = leaves[blockIdx.x];
    const int lane = threadIdx.x, bn = lf.bn, b0 = lf.b0;
    if (bn == 1) {
        if (lane == 0) {
            Q[b0 + (int64_t)b0 * n] = 1.0;
            lam[b0] = d[b0];
        }
        return;
    }
    for (int c = 0; c < bn; ++c) Qs[c * 64 + lane] = c == lane ? 1.0 : 0.0;
    double dr = lane < bn ? d[b0 + lane] : 0.0;
    double er = lane < bn - 1 ? e[b0 + lane] : 0.0;
    int capped = 0;
    for (int l = 0; l < bn; ++l) {
        for (int iter = 0;; ++iter) {
            int m = l;
            for (; m < bn - 1; ++m) {
                const double dd = fabs(dc_lane(dr, m)) + fabs(dc_lane(dr, m + 1));
                if (fabs(dc_lane(er, m)) <= DBL_EPSILON * dd) break;
            }
            if (m == l) break;
            if (iter >= kDcLeafSweeps) {
                ++capped;
                break;
            }
            const double dl = dc_lane(dr, l), el = dc_lane(er, l);
            double g = (dc_lane(dr, l + 1) - dl) / (2.0 * el);
            double r = hypot(g, 1.0);
            g = dc_lane(dr, m) - dl + el / (g + copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i = m - 1;
            for (; i >= l; --i) {
                const double ei = dc_lane(er, i);
                double f = s * ei;
                const double b = c * ei;
                r = hypot(f, g);
                if (lane == i + 1) er = r;
                if (r == 0.0) {
                    if (lane == i + 1) dr -= p;
                    if (lane == m) er = 0.0;
                    break;
                }
                s = f / r;
                c = g / r;
                g = dc_lane(dr, i + 1) - p;
                r = (dc_lane(dr, i) - g) * s + 2.0 * c * b;
                p = s * r;
                if (lane == i + 1) dr = g + p;
                g = c * r - b;
                f = Qs[(i + 1) * 64 + lane];
                const double q = Qs[i * 64 + lane];
                Qs[(i + 1) * 64 + lane] = s * q + c * f;
                Qs[i * 64 + lane] = c * q - s * f;
            }
            if (r == 0.0 && i >= l) continue;
            if (lane == l) {
                dr -= p;
                er = g;
            }
            if (lane == m) er = 0.0;
        }
    }
    if (lane < bn) {
        lam[b0 + lane] = dr;
        for (int c = 0; c < bn; ++c) Q[(b0 + lane) + (int64_t)(b0 + c) * n] = Qs[c * 64 + lane];
    }
    if (lane == 0 && capped) atomicAdd(ncap, capped);
}

// z_i = Q(zrow_i, i) for the columns of this level's merges (zrow_i < 0: not in a merge)
__global__ __launch_bounds__(256) void dc_gather_z(int n, const double* Q, const int* zrow, double* z) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = zrow[i];
    z[i] = r >= 0 ? Q[r + (int64_t)i * n] : 0.0;
}

// grid (row chunks, merges): thread = one row of the merge's block, the rotations in list order
__global__ __launch_bounds__(256) void dc_rotate(int n, double* Q, const DcMerge* merges, const DcRot* rots) {
    const DcMerge M = merges[blockIdx.y];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M.n) return;
    double* row = Q + M.lo + r;
    for (int q = M.rot0; q < M.rot0 + M.nrot; ++q) {
        const DcRot R = rots[q];
        const double x = row[(int64_t)R.a * n], y = row[(int64_t)R.b * n];
        row[(int64_t)R.a * n] = R.c * x + R.s * y;
        row[(int64_t)R.b * n] = R.c * y - R.s * x;
    }
}

// one workgroup per column of the level: dst(:, c) = src(:, from_c) over the merge's rows
__global__ __launch_bounds__(256) void dc_permute(int n, const double* src, double* dst, const DcMerge* merges,
                                                  const int* merge_of, const int* from) {
    const int c = blockIdx.x;
    const int mi = merge_of[c];
    if (mi < 0) return;
    const DcMerge M = merges[mi];
    const double* s = src + M.lo + (int64_t)from[c] * n;
    double* t = dst + M.lo + (int64_t)c * n;
    for (int r = threadIdx.x; r < M.n; r += 256) t[r] = s[r];
}

// the deflated columns (places k .. n of the merge) back from the permuted matrix
__global__ __launch_bounds__(256) void dc_copy_deflated(int n, const double* src, double* dst, const DcMerge* merges,
                                                        const int* merge_of) {
    const int c = blockIdx.x;
    const int mi = merge_of[c];
    if (mi < 0) return;
    const DcMerge M = merges[mi];
    if (c - M.lo < M.k) return;
    const double* s = src + M.lo + (int64_t)c * n;
    double* t = dst + M.lo + (int64_t)c * n;
    for (int r = threadIdx.x; r < M.n; r += 256) t[r] = s[r];
}

// sum_j z2_j / ((p_j - po) - x) over the k poles, in pole order; every lane of the wave calls it
__device__ __forceinline__ double dc_secular_sum(const double* P, const double* Z, int k, double po, double x,
                                                 double* sp, double* sz, int lane) {
    double s = 0.0;
    for (int c0 = 0; c0 < k; c0 += kDcChunk) {
        const int len = min(kDcChunk, k - c0);
        __syncthreads();
        for (int t = lane; t < len; t += 64) {
            sp[t] = P[c0 + t];
            const double zv = Z[c0 + t];
            sz[t] = zv * zv;
        }
        __syncthreads();
        for (int t = 0; t < len; ++t) s += sz[t] / ((sp[t] - po) - x);
    }
    return s;
}

// grid (ceil(kmax / 64), merges), one lane per root i of 1 + rho sum_j z_j^2 / (p_j - x) = 0, which lies in
// (p_i, p_{i+1}) (the last one in (p_{k-1}, p_{k-1} + rho |z|^2]).  The origin is the nearer pole: p_i when
// f((p_i + p_{i+1}) / 2) > 0, else p_{i+1}; nu = |x - origin| by bisection in (0, half the gap]: m = 2^-20 b
// while the lower end is 0, sqrt(a b) while b > 4 a, else the midpoint, until the bracket cannot be halved.
// porig_i = the origin pole, mu_i = +-nu, lam_i = porig_i + mu_i.
__global__ __launch_bounds__(64) void dc_secular(const DcMerge* merges, const double* pole, const double* zk, double* porig,
                                                 double* mu, double* lam, int* ncap) {
    __shared__ double sp[kDcChunk], sz[kDcChunk];
    const DcMerge M = merges[blockIdx.y];
    const int k = M.k;
    if ((int)blockIdx.x * 64 >= k) return;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < k;
    const double* P = pole + M.lo;
    const double* Z = zk + M.lo;
    const double rho = M.rho;
    if (k == 1) {
        if (lane == 0) {
            const double m1 = rho * Z[0] * Z[0];
            porig[M.lo] = P[0];
            mu[M.lo] = m1;
            lam[M.lo] = P[0] + m1;
        }
        return;
    }
    const int ii = active ? i : k - 1;
    const bool last = ii == k - 1;
    const double pi = P[ii];
    double half;
    {
        // |z|^2 in pole order (x = -1 and po = p_j is not a pole sum: take it directly)
        double nrm2 = 0.0;
        for (int c0 = 0; c0 < k; c0 += kDcChunk) {
            const int len = min(kDcChunk, k - c0);
            __syncthreads();
            for (int t = lane; t < len; t += 64) {
                const double zv = Z[c0 + t];
                sz[t] = zv * zv;
            }
            __syncthreads();
            for (int t = 0; t < len; ++t) nrm2 += sz[t];
        }
        half = last ? rho * nrm2 : 0.5 * (P[ii + 1] - pi);
    }
    const double fm = 1.0 + rho * dc_secular_sum(P, Z, k, pi, half, sp, sz, lane);
    const bool right = !last && fm <= 0.0;
    const double po = right ? P[ii + 1] : pi;
    const double sgn = right ? -1.0 : 1.0;
    double a = 0.0, b = half;
    bool live = active;
    int it = 0;
    for (; it < kDcSecularCap; ++it) {
        double m = a + 0.5 * (b - a);
        if (a == 0.0) {
            m = b * 0x1p-20;
        } else if (b > 4.0 * a) {   // sqrt(a b), not sqrt(a) sqrt(b): exact under a power-of-two scaling of T
            const double gm = sqrt(a * b);
            if (a < gm && gm < b) m = gm;
        }
        live = live && a < m && m < b;
        if (!__any(live)) break;
        const double g = 1.0 + rho * dc_secular_sum(P, Z, k, po, sgn * (live ? m : b), sp, sz, lane);
        if (live) {
            const bool up = right ? g > 0.0 : g <= 0.0;   // the root's nu is above m
            if (up) a = m;
            else b = m;
        }
    }
    if (active) {
        const double nu = a == 0.0 ? b : a + 0.5 * (b - a);
        porig[M.lo + i] = po;
        mu[M.lo + i] = sgn * nu;
        lam[M.lo + i] = po + sgn * nu;
        if (live && it >= kDcSecularCap) atomicAdd(ncap, 1);
    }
}

// grid (ceil(kmax / 64), merges), one lane per j: zhat_j = sign(z_j) sqrt(|w_j| / rho),
// w_j = (lam_j - p_j) prod_{i != j} (lam_i - p_j) / (p_i - p_j) as a running product in i order,
// lam_i - p_j formed as (porig_i - p_j) + mu_i.
__global__ __launch_bounds__(64) void dc_loewner(const DcMerge* merges, const double* pole, const double* zk,
                                                 const double* porig, const double* mu, double* zhat) {
    __shared__ double sp[kDcChunk], so[kDcChunk], sm[kDcChunk];
    const DcMerge M = merges[blockIdx.y];
    const int k = M.k;
    if ((int)blockIdx.x * 64 >= k) return;
    const int lane = threadIdx.x;
    const int j = blockIdx.x * 64 + lane;
    const bool active = j < k;
    const int jj = active ? j : k - 1;
    const double pj = pole[M.lo + jj];
    double w = (porig[M.lo + jj] - pj) + mu[M.lo + jj];
    for (int c0 = 0; c0 < k; c0 += kDcChunk) {
        const int len = min(kDcChunk, k - c0);
        __syncthreads();
        for (int t = lane; t < len; t += 64) {
            sp[t] = pole[M.lo + c0 + t];
            so[t] = porig[M.lo + c0 + t];
            sm[t] = mu[M.lo + c0 + t];
        }
        __syncthreads();
        for (int t = 0; t < len; ++t) {
            const double ratio = ((so[t] - pj) + sm[t]) / (sp[t] - pj);
            w *= (c0 + t) == jj ? 1.0 : ratio;
        }
    }
    if (active) {
        const double v = sqrt(fabs(w) / M.rho);
        zhat[M.lo + j] = zk[M.lo + j] < 0.0 ? -v : v;
    }
}

// grid (kmax, merges), one workgroup per column i of U (k x k at U + lo + lo n, leading dimension n):
// u_ji = zhat_j / ((p_j - porig_i) - mu_i), then the column scaled to unit 2-norm (the squares summed per
// thread in j order, the 256 partial sums by a tree: a fixed order).
__global__ __launch_bounds__(256) void dc_vectors(int n, const DcMerge* merges, const double* pole, const double* zhat,
                                                  const double* porig, const double* mu, double* U) {
    __shared__ double red[256];
    const DcMerge M = merges[blockIdx.y];
    const int k = M.k, i = blockIdx.x;
    if (i >= k) return;
    const double po = porig[M.lo + i], m = mu[M.lo + i];
    double* u = U + M.lo + (int64_t)(M.lo + i) * n;
    double ss = 0.0;
    for (int j = threadIdx.x; j < k; j += 256) {
        const double v = zhat[M.lo + j] / ((pole[M.lo + j] - po) - m);
        u[j] = v;
        ss += v * v;
    }
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double scl = 1.0 / sqrt(red[0]);
    for (int j = threadIdx.x; j < k; j += 256) u[j] *= scl;
}

// ZT(:, j) = Q(:, cols_j)
__global__ __launch_bounds__(256) void dc_take_columns(int n, const double* Q, const int* cols, double* ZT) {
    const double* s = Q + (int64_t)cols[blockIdx.x] * n;
    double* t = ZT + (int64_t)blockIdx.x * n;
    for (int r = threadIdx.x; r < n; r += 256) t[r] = s[r];
}

}  // namespace dev

// ============================================================================ host
namespace {

constexpr double kUnitRoundoff = 0x1p-53;   // dlamch('E')

struct DeflateOut {
    int64_t k = 0;
    double rho = 0.0, tol = 0.0;
    std::vector<int64_t> perm;
    std::vector<double> dk, zk;
    std::vector<int64_t> rot_cols;
    std::vector<double> rot_cs;
};

// dlaed2's deflation; see eigsol_dc_deflate in eigsol_hip.h
void dc_deflate_host(int64_t n, const double* d_in, const double* z_in, double rho, DeflateOut& o) {
    std::vector<double> d(d_in, d_in + n), z(z_in, z_in + n);
    double nrm2 = 0.0;
    for (int64_t j = 0; j < n; ++j) nrm2 += z[j] * z[j];
    const double nrm = std::sqrt(nrm2);
    if (nrm > 0.0)
        for (int64_t j = 0; j < n; ++j) z[j] = z[j] / nrm;
    rho = rho * nrm2;
    std::vector<int64_t> order(n);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return d[a] < d[b]; });
    double dmax = 0.0, zmax = 0.0;
    for (int64_t j = 0; j < n; ++j) {
        dmax = std::max(dmax, std::fabs(d[j]));
        zmax = std::max(zmax, std::fabs(z[j]));
    }
    const double tol = 8.0 * kUnitRoundoff * std::max(dmax, zmax);
    std::vector<int64_t> kept, gone;
    o.rot_cols.clear();
    o.rot_cs.clear();
    if (rho * zmax <= tol) {
        gone = order;
    } else {
        int64_t pj = -1;
        for (int64_t q = 0; q < n; ++q) {
            const int64_t j = order[q];
            if (rho * std::fabs(z[j]) <= tol) {
                gone.push_back(j);
            } else if (pj < 0) {
                pj = j;
            } else {
                double s = z[pj], c = z[j];
                const double tau = std::hypot(c, s);
                double t = d[j] - d[pj];
                c = c / tau;
                s = -s / tau;
                if (std::fabs(t * c * s) <= tol) {
                    z[j] = tau;
                    z[pj] = 0.0;
                    o.rot_cols.push_back(pj);
                    o.rot_cols.push_back(j);
                    o.rot_cs.push_back(c);
                    o.rot_cs.push_back(s);
                    t = d[pj] * c * c + d[j] * s * s;
                    d[j] = d[pj] * s * s + d[j] * c * c;
                    d[pj] = t;
                    gone.push_back(pj);
                } else {
                    kept.push_back(pj);
                }
                pj = j;
            }
        }
        kept.push_back(pj);
    }
    o.k = (int64_t)kept.size();
    o.rho = rho;
    o.tol = tol;
    o.perm = kept;
    o.perm.insert(o.perm.end(), gone.begin(), gone.end());
    o.dk.resize(n);
    o.zk.assign(n, 0.0);
    for (int64_t q = 0; q < n; ++q) o.dk[q] = d[o.perm[q]];
    for (int64_t q = 0; q < o.k; ++q) o.zk[q] = z[o.perm[q]];
}

struct DcNode {
    int lo, n, n1;     // rows [lo, lo + n); the left half has n1 rows (0: a leaf)
    int left, right;   // children (-1: a leaf)
    int height;
    double rho;
};

int dc_build(std::vector<DcNode>& nodes, std::vector<double>& d, const double* e, int lo, int n, int leaf) {
    DcNode nd{lo, n, 0, -1, -1, 0, 0.0};
    if (n > leaf) {
        nd.n1 = n / 2;
        const int c = lo + nd.n1 - 1;
        nd.rho = e[c];
        d[c] -= nd.rho;
        d[c + 1] -= nd.rho;
        nd.left = dc_build(nodes, d, e, lo, nd.n1, leaf);
        nd.right = dc_build(nodes, d, e, lo + nd.n1, n - nd.n1, leaf);
        nd.height = 1 + std::max(nodes[nd.left].height, nodes[nd.right].height);
    }
    nodes.push_back(nd);
    return (int)nodes.size() - 1;
}

int dc_leaf_order() {
    int leaf = dev::kDcLeafMax;
    if (const char* s = std::getenv("EIGSOL_DC_LEAF")) {
        const int v = std::atoi(s);
        if (v >= 2 && v <= dev::kDcLeafMax) leaf = v;
    }
    return leaf;
}

}  // namespace

int eigh_dc_tridiag(eigsol_ctx* ctx, int64_t n64, const double* d_in, const double* e_in, const std::vector<int64_t>& starts,
                    DevBuf& dQ, double* lam, int64_t* ncap_out) {
    using namespace dev;
    hipStream_t st = ctx->stream;
    const int n = (int)n64;
    const int leaf = dc_leaf_order();
    // ---- every split block scaled by the power of two that brings its largest |d_i|, e_i into [1, 2) (dstedc
    // scales to unit max-norm for the same reason): dlaed2's tol = 8 u max(max |d|, max |z|) takes |z| <= 1 as
    // the scale of the poles, so on a block of small norm it would deflate couplings that matter.  Exact, and
    // undone on the eigenvalues at the end; 2^k T then gives the bits of T.
    std::vector<double> d(d_in, d_in + n), es(std::max(n, 1), 0.0);
    std::vector<int> kexp(n, 0);   // per row: its block's exponent
    for (size_t b = 0; b + 1 < starts.size(); ++b) {
        const int b0 = (int)starts[b], b1 = (int)starts[b + 1];
        double amax = 0.0;
        for (int i = b0; i < b1; ++i) {
            amax = std::max(amax, std::fabs(d[i]));
            if (i + 1 < b1) amax = std::max(amax, std::fabs(e_in[i]));
        }
        const int k = amax > 0.0 ? -std::ilogb(amax) : 0;
        for (int i = b0; i < b1; ++i) {
            kexp[i] = k;
            d[i] = std::ldexp(d[i], k);
            if (i + 1 < b1) es[i] = std::ldexp(e_in[i], k);
        }
    }
    const double* e = es.data();
    // ---- plan
    std::vector<DcNode> nodes;
    int H = 0;
    for (size_t b = 0; b + 1 < starts.size(); ++b) {
        const int root = dc_build(nodes, d, e, (int)starts[b], (int)(starts[b + 1] - starts[b]), leaf);
        H = std::max(H, nodes[root].height);
    }
    std::vector<DcLeaf> leaves;
    std::vector<std::vector<int>> by_height(H + 1);
    for (int q = 0; q < (int)nodes.size(); ++q) {
        if (nodes[q].left < 0) leaves.push_back(DcLeaf{nodes[q].lo, nodes[q].n});
        else by_height[nodes[q].height].push_back(q);
    }
    const size_t nn = (size_t)n * n;
    DevBuf dB, dU, dd, de, dlam, dz, dzrow, dfrom, dmof, dpole, dzk, dporig, dmu, dzh, dmerges, drots, dleaves, dcap;
    EIGSOL_TRY(dQ.alloc(nn * sizeof(double)));
    EIGSOL_TRY(dd.alloc((size_t)n * sizeof(double)));
    EIGSOL_TRY(de.alloc((size_t)n * sizeof(double)));
    EIGSOL_TRY(dlam.alloc((size_t)n * sizeof(double)));
    EIGSOL_TRY(dleaves.alloc(leaves.size() * sizeof(DcLeaf)));
    EIGSOL_TRY(dcap.alloc(64));
    if (H > 0) {
        EIGSOL_TRY(dB.alloc(nn * sizeof(double)));
        EIGSOL_TRY(dU.alloc(nn * sizeof(double)));
        for (DevBuf* b : {&dz, &dpole, &dzk, &dporig, &dmu, &dzh}) EIGSOL_TRY(b->alloc((size_t)n * sizeof(double)));
        for (DevBuf* b : {&dzrow, &dfrom, &dmof}) EIGSOL_TRY(b->alloc((size_t)n * sizeof(int)));
        EIGSOL_TRY(dmerges.alloc((size_t)(n / 2 + 1) * sizeof(DcMerge)));
        EIGSOL_TRY(drots.alloc((size_t)n * sizeof(DcRot)));
    }
    StageClock clock;   // marks 0, 1 around the leaves; level h: 3 h - 1 .. 3 h + 1 around its vector kernels and its GEMMs
    EIGSOL_TRY(clock.start(1 + 3 * H));
    EIGSOL_TRY(clock.mark(0, st));
    EIGSOL_HIP(hipMemsetAsync(dQ.p, 0, nn * sizeof(double), st));
    EIGSOL_HIP(hipMemsetAsync(dcap.p, 0, 64, st));
    EIGSOL_HIP(hipMemcpyAsync(dd.p, d.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    if (n > 1) EIGSOL_HIP(hipMemcpyAsync(de.p, e, (size_t)(n - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dleaves.p, leaves.data(), leaves.size() * sizeof(DcLeaf), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dc_leaf, dim3((unsigned)leaves.size()), dim3(64), 0, st, n, dd.as<double>(), de.as<double>(),
                       dleaves.as<DcLeaf>(), dQ.as<double>(), dlam.as<double>(), dcap.as<int>());
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_TRY(clock.mark(1, st));

    // ---- merges, level by level
    double host_ms = 0.0;
    std::vector<double> z(n);
    std::vector<int> zrow(n), from(n), mof(n);
    std::vector<double> pole(n), zk(n);
    std::vector<DcMerge> merges;
    std::vector<DcRot> rots;
    DeflateOut D;
    const unsigned gn = (unsigned)((n + 255) / 256);
    for (int h = 1; h <= H; ++h) {
        const std::vector<int>& lv = by_height[h];
        std::fill(zrow.begin(), zrow.end(), -1);
        for (int q : lv) {
            const DcNode& nd = nodes[q];
            for (int c = nd.lo; c < nd.lo + nd.n1; ++c) zrow[c] = nd.lo + nd.n1 - 1;
            for (int c = nd.lo + nd.n1; c < nd.lo + nd.n; ++c) zrow[c] = nd.lo + nd.n1;
        }
        EIGSOL_HIP(hipMemcpyAsync(dzrow.p, zrow.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(dc_gather_z, dim3(gn), dim3(256), 0, st, n, dQ.as<double>(), dzrow.as<int>(), dz.as<double>());
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_HIP(hipMemcpyAsync(z.data(), dz.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(lam, dlam.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipStreamSynchronize(st));   // the level's one host wait; the last level's uploads are done too
        auto w2 = std::chrono::steady_clock::now();
        merges.clear();
        rots.clear();
        std::fill(mof.begin(), mof.end(), -1);
        int kmax = 0, nmax = 0;
        for (int q : lv) {
            const DcNode& nd = nodes[q];
            dc_deflate_host(nd.n, lam + nd.lo, z.data() + nd.lo, nd.rho, D);
            DcMerge M{nd.lo, nd.n, (int)D.k, (int)rots.size(), (int)(D.rot_cols.size() / 2), 0, D.rho};
            for (int r = 0; r < M.nrot; ++r)
                rots.push_back(DcRot{nd.lo + (int)D.rot_cols[2 * r], nd.lo + (int)D.rot_cols[2 * r + 1], D.rot_cs[2 * r],
                                     D.rot_cs[2 * r + 1]});
            for (int p = 0; p < nd.n; ++p) {
                lam[nd.lo + p] = D.dk[p];
                pole[nd.lo + p] = D.dk[p];
                zk[nd.lo + p] = D.zk[p];
                from[nd.lo + p] = nd.lo + (int)D.perm[p];
                mof[nd.lo + p] = (int)merges.size();
            }
            kmax = std::max(kmax, M.k);
            nmax = std::max(nmax, M.n);
            merges.push_back(M);
        }
        const unsigned nm = (unsigned)merges.size();
        auto w3 = std::chrono::steady_clock::now();
        host_ms += std::chrono::duration<double, std::milli>(w3 - w2).count();
        // the host arrays below are next written after the next level's wait (or freed after the final one)
        EIGSOL_HIP(hipMemcpyAsync(dmerges.p, merges.data(), nm * sizeof(DcMerge), hipMemcpyHostToDevice, st));
        if (!rots.empty())
            EIGSOL_HIP(hipMemcpyAsync(drots.p, rots.data(), rots.size() * sizeof(DcRot), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dfrom.p, from.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dmof.p, mof.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dpole.p, pole.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dzk.p, zk.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(dlam.p, lam, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        EIGSOL_TRY(clock.mark(3 * h - 1, st));
        if (!rots.empty())
            hipLaunchKernelGGL(dc_rotate, dim3((unsigned)((nmax + 255) / 256), nm), dim3(256), 0, st, n, dQ.as<double>(),
                               dmerges.as<DcMerge>(), drots.as<DcRot>());
        hipLaunchKernelGGL(dc_permute, dim3((unsigned)n), dim3(256), 0, st, n, dQ.as<double>(), dB.as<double>(),
                           dmerges.as<DcMerge>(), dmof.as<int>(), dfrom.as<int>());
        if (kmax > 0) {
            const unsigned gk = (unsigned)((kmax + 63) / 64);
            hipLaunchKernelGGL(dc_secular, dim3(gk, nm), dim3(64), 0, st, dmerges.as<DcMerge>(), dpole.as<double>(),
                               dzk.as<double>(), dporig.as<double>(), dmu.as<double>(), dlam.as<double>(), dcap.as<int>());
            hipLaunchKernelGGL(dc_loewner, dim3(gk, nm), dim3(64), 0, st, dmerges.as<DcMerge>(), dpole.as<double>(),
                               dzk.as<double>(), dporig.as<double>(), dmu.as<double>(), dzh.as<double>());
            hipLaunchKernelGGL(dc_vectors, dim3((unsigned)kmax, nm), dim3(256), 0, st, n, dmerges.as<DcMerge>(),
                               dpole.as<double>(), dzh.as<double>(), dporig.as<double>(), dmu.as<double>(), dU.as<double>());
        }
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY(clock.mark(3 * h, st));
        // one GEMM launch per merge: Q(rows, kept) = B(rows, kept) U
        for (const DcMerge& M : merges) {
            if (M.k == 0) continue;
            const int64_t off = M.lo + (int64_t)M.lo * n;
            EIGSOL_TRY(hess_gemm_nn_f64(st, M.n, M.k, M.k, dB.as<double>() + off, n, dU.as<double>() + off, n,
                                        dQ.as<double>() + off, n));
        }
        hipLaunchKernelGGL(dc_copy_deflated, dim3((unsigned)n), dim3(256), 0, st, n, dB.as<double>(), dQ.as<double>(),
                           dmerges.as<DcMerge>(), dmof.as<int>());
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY(clock.mark(3 * h + 1, st));
    }
    int ncap = 0;
    EIGSOL_HIP(hipMemcpyAsync(lam, dlam.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&ncap, dcap.p, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) lam[i] = std::ldexp(lam[i], -kexp[i]);   // back to T's scale, exactly
    *ncap_out = ncap;
    std::vector<double> ms(1 + 3 * H);
    clock.read(ms.data(), 1 + 3 * H);
    double vec_ms = 0.0, gemm_ms = 0.0;
    ctx->eigh_dc_ms[1] = ms[0];
    for (int h = 1; h <= H; ++h) {
        vec_ms += ms[3 * h - 1];
        gemm_ms += ms[3 * h];
    }
    ctx->eigh_dc_ms[2] = host_ms;
    ctx->eigh_dc_ms[3] = vec_ms;
    ctx->eigh_dc_ms[4] = gemm_ms;
    return EIGSOL_OK;
}

int eigh_dc_take_columns(hipStream_t st, int64_t n, int64_t m, const double* Q, const std::vector<int>& cols, double* ZT) {
    if (m <= 0) return EIGSOL_OK;
    DevBuf dcols;
    EIGSOL_TRY(dcols.alloc((size_t)m * sizeof(int)));
    EIGSOL_HIP(hipMemcpyAsync(dcols.p, cols.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dev::dc_take_columns, dim3((unsigned)m), dim3(256), 0, st, (int)n, Q, dcols.as<int>(), ZT);
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipStreamSynchronize(st));   // dcols and cols go out of scope
    return EIGSOL_OK;
}

}  // namespace eigsol

using namespace eigsol;

extern "C" int eigsol_dc_deflate(int64_t n, int64_t n1, const double* d, const double* z, double rho, int64_t* k_out,
                                 int64_t* perm, double* dk, double* zk, double* rho_out, int64_t* nrot_out,
                                 int64_t* rot_cols, double* rot_cs, double* tol_out) {
    if (!d || !z || !k_out || !perm || !dk || !zk || !rho_out || !nrot_out || !rot_cols || !rot_cs)
        return fail(EIGSOL_E_INVALID, "eigsol_dc_deflate: null pointer");
    if (n < 2 || n1 < 1 || n1 >= n) return fail(EIGSOL_E_INVALID, "eigsol_dc_deflate: needs n >= 2 and 1 <= n1 < n");
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(EIGSOL_E_INVALID, "eigsol_dc_deflate: rho must be positive and finite");
    for (int64_t j = 0; j < n; ++j)
        if (!std::isfinite(d[j]) || !std::isfinite(z[j])) return fail(EIGSOL_E_INVALID, "eigsol_dc_deflate: non-finite input");
    DeflateOut D;
    dc_deflate_host(n, d, z, rho, D);
    *k_out = D.k;
    *rho_out = D.rho;
    if (tol_out) *tol_out = D.tol;
    *nrot_out = (int64_t)D.rot_cols.size() / 2;
    for (int64_t q = 0; q < n; ++q) {
        perm[q] = D.perm[q];
        dk[q] = D.dk[q];
        zk[q] = D.zk[q];
    }
    for (size_t q = 0; q < D.rot_cols.size(); ++q) {
        rot_cols[q] = D.rot_cols[q];
        rot_cs[q] = D.rot_cs[q];
    }
    return EIGSOL_OK;
}
