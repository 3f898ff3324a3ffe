// The sparse level-ordered triangular solve of the shifted-solve family on gfx950 (config 5): the factor IS the
// matrix.  Pivots d_i - sigma (coeffRef inserts a missing diagonal, solve_shifted.hpp:100-102), rows ordered by
// dependency level, and a sync-free solve: each 16-lane group solves one row, polling the solved values of the rows
// it reads (an unsolved value is a sentinel NaN).
//
// This file holds the kernels' argument struct (TriArgs), the sentinel and the row-group reductions, the head,
// wave-head, slice, chunk and chunk-role kernels, the partials kernels (also launched for the GMRES family's
// iteration, iter_decide_launch / iter_part_launch), the launch geometry (tri_launch_setup) and the launch
// (tri_launch).  The factor's analysis and layout live in tri_factor.hip, the factor object in shift_factor.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "shift_factor.hpp"
#include "solve_poll.hpp"

namespace eigsol {

static constexpr int kMultiDefault = 4;   // EIGSOL_TRSV_MULTI (config 5 per iteration: K = 1 0.674, 2 0.502, 3 0.439, 4 0.414 ms)

namespace dev {

constexpr int kSpinLimit = 1 << 20;   // polls (with back-off) before the wait is declared broken

template <class S>
struct TriArgs {
    const int32_t* order;  // head position -> row
    const S* hval;         // head, pass-major: entry k of group g of pass q at (q * 64 + g) * 16 + k
    const int32_t* hcol;   // LDS position of the column (padding: the zero slot hpos)
    const S* hpiv;         // pivot of group g of pass q at q * 64 + g
    const int2* passes;    // head passes
    int32_t npass, hpos;   // head passes, head positions
    const S* wval;         // one-wave head: entry k of lane l of pass q at (q * 4 + k) * 64 + l
    const int32_t* wcol;   // its LDS column position (padding: the zero slot hpos)
    const S* wrp;          // 1 / pivot of row group g of pass q at q * 16 + g
    const int32_t* wdst;   // LDS position that group g of pass q solves (-1: none)
    int32_t nwpass;
    const int2* smeta;     // tail slices: {entry offset, entries per lane}
    const int32_t* trow;   // row of lane l of slice s at s * 64 + l (-1: padding)
    const S* tpiv;
    const int32_t* tcol;   // entry k of lane l of slice s at off + 64 k + l (padding: the zero slot n)
    const S* tval;
    int32_t nslices;
    const int32_t* porder; // chunk variant, position-indexed: row (-1: padding), entries, pivots
    const int32_t* pptr;
    const int32_t* pcol;
    const S* pval;
    const S* ppiv;
    int32_t chunk0, nchunks;
    int32_t poll_fast;     // tail: polls re-issued without back-off
    int32_t poll_mode;     // bit 0: slice tail re-polls one dependency per lane; bit 1: late second-chunk polls
    int64_t n;
    S* zcur;            // polled by this launch
    S* znext;           // reset to the sentinel by this launch, for the next one
    uint32_t* work;
    int32_t* err;
    part4* wave_part;
    const S* b_plain;   // solve mode
    S* y_plain;
    S* buf0;            // iteration mode (same parity convention as the power loop)
    S* buf1;
    PowerCtl* ctl;
    const part4* rank_part;
    part4* my_part;
    S* trace;
    double sig_re, sig_im;
    // multi-solve launches (K solves; solve 0 polls zcur)
    int32_t K;
    S* zk[kMaxMulti];   // solve j's polled values (zk[0] = zcur)
    S* zkn[kMaxMulti];  // ... and the next launch's buffers (zkn[0] = znext)
    S* aux[kMaxMulti - 1];   // w_0 .. w_{K-2}
    part4* kpart;       // solves 1..K-1: {||w_j||^2, w_{j-1}^H w_j}
    part4* kblk;        // (K - 1) x red_grid block partials
    int32_t hconc;      // multi head: the K solves concurrently (K LDS value arrays)
};

// multiplication by an exact power of two (the pair launch's scaling of w1)
__device__ __forceinline__ double scale_r(double v, double s) { return v * s; }
__device__ __forceinline__ cplx scale_r(cplx v, double s) { return cplx{v.re * s, v.im * s}; }
__device__ __forceinline__ float scale_r(float v, double s) { return v * (float)s; }
__device__ __forceinline__ cplxf scale_r(cplxf v, double s) { return cplxf{v.re * (float)s, v.im * (float)s}; }

__device__ __forceinline__ int ld_flag_err(const int32_t* p) {
    return __hip_atomic_load(const_cast<int32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool unready(double v) { return (unsigned long long)__double_as_longlong(v) == kSent; }
__device__ __forceinline__ bool unready(cplx v) { return unready(v.re) || unready(v.im); }
// single precision: every 32-bit word of an unsolved entry holds the low word of kSent (a NaN)
__device__ __forceinline__ bool unready(float v) { return __float_as_uint(v) == (uint32_t)(kSent & 0xffffffffu); }
__device__ __forceinline__ bool unready(cplxf v) { return unready(v.re) || unready(v.im); }
__device__ __forceinline__ double sanitize(double v) {
    return unready(v) ? __longlong_as_double(0x7FF8000000000000ll) : v;
}
__device__ __forceinline__ cplx sanitize(cplx v) { return cplx{sanitize(v.re), sanitize(v.im)}; }
__device__ __forceinline__ float sanitize(float v) { return unready(v) ? __uint_as_float(0x7FC00000u) : v; }
__device__ __forceinline__ cplxf sanitize(cplxf v) { return cplxf{sanitize(v.re), sanitize(v.im)}; }
template <class S>
__device__ __forceinline__ S sentinel() {
    const double s = __longlong_as_double((long long)kSent);
    const float sf = __uint_as_float((uint32_t)(kSent & 0xffffffffu));
    if constexpr (std::is_same_v<S, double>) return s;
    else if constexpr (std::is_same_v<S, cplx>) return cplx{s, s};
    else if constexpr (std::is_same_v<S, float>) return sf;
    else return cplxf{sf, sf};
}
template <class S>
__device__ __forceinline__ S s_one() {
    if constexpr (std::is_same_v<S, double>) return 1.0;
    else if constexpr (std::is_same_v<S, cplx>) return cplx{1.0, 0.0};
    else if constexpr (std::is_same_v<S, float>) return 1.0f;
    else return cplxf{1.0f, 0.0f};
}

// sum over the 16 lanes of a row group.  16 lanes: a DPP butterfly over the lane-index xor
// masks 15 (row_mirror), 7 (row_half_mirror), 3 and 1 (quad_perm), which span all 16 lanes:
// four VALU steps instead of four LDS-latency ds_bpermute round trips, and every lane of the
// group ends with the same bits (each step adds the same two values in both lanes).
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int kCtrl>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xf, 0xf, false));
}
constexpr int kDppRowMirror = 0x140, kDppRowHalfMirror = 0x141, kDppQuad3210 = 0x1B, kDppQuad1032 = 0xB1;
__device__ __forceinline__ double group_sum(double v) {
    if constexpr (kRowLanes == 16) {
        v += dpp_f64<kDppRowMirror>(v);
        v += dpp_f64<kDppRowHalfMirror>(v);
        v += dpp_f64<kDppQuad3210>(v);
        v += dpp_f64<kDppQuad1032>(v);
    } else {
#pragma unroll
        for (int off = kRowLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    }
    return v;
}
__device__ __forceinline__ cplx group_sum(cplx v) { return cplx{group_sum(v.re), group_sum(v.im)}; }
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (kRowLanes == 16) {
        v += dpp_f32<kDppRowMirror>(v);
        v += dpp_f32<kDppRowHalfMirror>(v);
        v += dpp_f32<kDppQuad3210>(v);
        v += dpp_f32<kDppQuad1032>(v);
    } else {
#pragma unroll
        for (int off = kRowLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    }
    return v;
}
__device__ __forceinline__ cplxf group_sum(cplxf v) { return cplxf{group_sum(v.re), group_sum(v.im)}; }

// poll z[j] until solved (bounded; a broken wait sets the sticky error word and gives up)
template <class S>
__device__ __forceinline__ S wait_value(const S* z, int j, int32_t* err) {
    S y = ld_cohi(z, j);
    int spins = 0;
    while (unready(y)) {
        // back off, exponentially: a wave far ahead of the dependency frontier must leave the
        // memory system to the producers
        if (spins < 4) __builtin_amdgcn_s_sleep(2);
        else if (spins < 16) __builtin_amdgcn_s_sleep(8);
        else __builtin_amdgcn_s_sleep(32);
        y = ld_cohi(z, j);
        if ((++spins & 255) == 0 && (spins > kSpinLimit || ld_flag_err(err) != 0)) {
            atomicOr(err, 1);
            break;
        }
    }
    return y;
}

// ---- head: the narrow leading levels, one workgroup, solved values in LDS.
// Levels [0, nhl) hold few rows each (the bottom of an upper-triangular DAG: the first 185 of
// config 5's 372 levels hold 9k of its 1M rows).  Through memory every level costs a coherent
// store + poll round trip (~1.1 us); here a level is a workgroup barrier and LDS reads.  Every
// column a head row reads is an earlier head row (lower level), so columns are LDS positions.
// Pass-major layout built at factor time: pass q (64 rows of one level, one per 16-lane group)
// stores entry k of its group g at hval/hcol[(q * 64 + g) * 16 + k] (padded: column -1) and the
// group's pivot at hpiv[q * 64 + g].  No load depends on another, so the loads of the next kHeadDepth
// passes are in flight (a register ring) while a pass computes: a pass costs its LDS and
// arithmetic latency, not a memory round trip.  zl starts as the scaled right-hand side.
// Padding entries read the zero slot zl[hpos] with value zero; the pass count is padded to a
// multiple of the ring depth with empty passes, so the ring loop is straight-line code.

template <class S, bool kIter>
__global__ __launch_bounds__(kHeadThreads) void sptrsv_head_kernel(TriArgs<S> a, int parity) {
    extern __shared__ __align__(16) unsigned char head_lds[];
    S* zl = reinterpret_cast<S*>(head_lds);
    // zl[hpos] is a zero (the column of padding entries, whose values are zero too)
    int2* pl = reinterpret_cast<int2*>(head_lds + (size_t)(a.hpos + 1) * sizeof(S));   // pass table
    __shared__ Prologue pro;
    const S* xin;
    S* yout;
    double nrm = 0.0;
    if constexpr (kIter) {
        shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) return;   // the tail kernel resets z
        nrm = pro.nrm;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    const int tid = threadIdx.x;
    const int lane = tid & (kRowLanes - 1);
    const int grp = tid / kRowLanes;
    const int npass = a.npass;
    S rv[kHeadDepth], rp[kHeadDepth];
    int rc[kHeadDepth];
    auto load = [&](int q, S& v, int& c, S& p) {
        const uint32_t e = (uint32_t)(q < npass ? q : 0) * kHeadThreads + (uint32_t)tid;
        v = ldg_stream(a.hval, e);
        c = (int)ldg_stream(a.hcol, e);
        p = ldg_stream(a.hpiv, (uint32_t)(q < npass ? q : 0) * kHeadRows + (uint32_t)grp);
    };
#pragma unroll
    for (int u = 0; u < kHeadDepth; ++u) load(u, rv[u], rc[u], rp[u]);
    for (int p = tid; p < a.hpos; p += kHeadThreads) {
        const int i = a.order[p];
        S b = xin[i >= 0 ? i : 0];
        if constexpr (kIter) b = scale_in(b, nrm);
        zl[p] = b;
    }
    if (tid == 0) zl[a.hpos] = s_zero<S>();
    for (int q = tid; q < npass; q += kHeadThreads) pl[q] = a.passes[q];
    __syncthreads();
    for (int q0 = 0; q0 < npass; q0 += kHeadDepth) {
#pragma unroll
        for (int u = 0; u < kHeadDepth; ++u) {   // straight line: npass is a multiple of the depth
            const int q = q0 + u;
            const int2 pb = pl[q];   // LDS: a vector load here would wait for the ring (vmcnt is in order)
            S acc = group_sum(mul(rv[u], zl[rc[u]]));
            const int pos = pb.x + grp;
            if (lane == 0 && pos < (pb.y & ~kPassBarrier)) zl[pos] = sdiv(sub(zl[pos], acc), rp[u]);
            if (pb.y & kPassBarrier) __syncthreads();
            load(q + kHeadDepth, rv[u], rc[u], rp[u]);
            asm volatile("" ::: "memory");   // keep the refills in ring order (vmcnt retires in issue order)
        }
    }
    __syncthreads();
    // publish: the tail kernel (next in stream order) reads these through z
    for (int p = tid; p < a.hpos; p += kHeadThreads) {
        const int i = a.order[p];
        if (i < 0) continue;
        const S yi = sanitize(zl[p]);
        a.zcur[i] = yi;
        yout[i] = yi;
        a.znext[i] = sentinel<S>();
    }
}

// ---- head, one-wave form.  The narrow levels are a chain of short dependent steps; with a
// workgroup, every pass costs a barrier and the instruction issue of 16 waves (~0.6 us for 64
// rows).  Here ONE wave solves them with no barrier at all (a wave's LDS operations complete in
// issue order): 4 lanes per row, 4 entries per lane, 16 rows per pass, and the row's pivot applied
// as a multiplication by its reciprocal (computed at factor time).  A pass never spans two levels,
// so the rows of a pass are independent; the entries of the next kWHeadDepth passes are in flight
// in a register ring.  The other waves only help to stage the right-hand side into LDS and to
// publish the solved values.
constexpr int kWHeadThreads = 256;
constexpr int kDppQuad2301 = 0x4E;
__device__ __forceinline__ double quad_sum(double v) {
    v += dpp_f64<kDppQuad1032>(v);
    return v + dpp_f64<kDppQuad2301>(v);
}
__device__ __forceinline__ float quad_sum(float v) {
    v += dpp_f32<kDppQuad1032>(v);
    return v + dpp_f32<kDppQuad2301>(v);
}
__device__ __forceinline__ cplx quad_sum(cplx v) { return cplx{quad_sum(v.re), quad_sum(v.im)}; }
__device__ __forceinline__ cplxf quad_sum(cplxf v) { return cplxf{quad_sum(v.re), quad_sum(v.im)}; }

// kMulti: the multi-solve launch's head (shift_multi_prologue): the head is solved K times from
// LDS, solve j on s * (solve j-1's solution); solve j is published to zk[j] and, for the last
// one, to B[parity] (the earlier ones to aux[j]).
template <class S, bool kIter, bool kMulti = false>
__global__ __launch_bounds__(kWHeadThreads) void sptrsv_whead_kernel(TriArgs<S> a, int parity) {
    extern __shared__ __align__(16) unsigned char head_lds[];
    S* zl = reinterpret_cast<S*>(head_lds);
    __shared__ Prologue pro;
    const S* xin;
    S* yout;
    double nrm = 0.0, s2 = 1.0;
    const int K = kMulti ? a.K : 1;
    if constexpr (kIter) {
        if constexpr (kMulti)
            shift_multi_prologue<S>(a.ctl, a.rank_part, a.kpart, a.K, parity, a.trace, a.sig_re, a.sig_im, &pro);
        else
            shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) return;   // the tail kernel resets z
        nrm = pro.nrm;
        s2 = pro.s;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    const int tid = threadIdx.x;
    // right-hand side of the head positions into LDS: 8 positions per thread per round, every
    // load of a round issued before the first is consumed
    constexpr int kB = 8;
    for (int p0 = 0; p0 < a.hpos; p0 += kWHeadThreads * kB) {
        int ii[kB];
        S bb[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int p = p0 + u * kWHeadThreads + tid;
            ii[u] = p < a.hpos ? a.order[p] : -1;
        }
#pragma unroll
        for (int u = 0; u < kB; ++u) bb[u] = xin[ii[u] >= 0 ? ii[u] : 0];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int p = p0 + u * kWHeadThreads + tid;
            if (p < a.hpos) {
                if constexpr (kIter) zl[p] = scale_in(bb[u], nrm);
                else zl[p] = bb[u];
            }
        }
    }
    // multi-solve launch, concurrent head (a.hconc: every solve's values fit the LDS): wave j
    // solves system j in its own LDS array, one pass behind wave j - 1: before pass q it waits
    // for wave j - 1's progress word (LDS operations of one wave execute in order, so a progress
    // value q + 1 means pass q's values are in place), then takes its right-hand side s w_{j-1}
    // from wave j - 1's array.
    const int64_t pitch = a.hpos + 1;
    volatile int* prog = reinterpret_cast<volatile int*>(zl + K * pitch);
    const bool conc = kMulti && a.hconc;
    if (tid == 0) {
        zl[a.hpos] = s_zero<S>();
        if (conc)
            for (int j = 1; j < K; ++j) {
                zl[j * pitch + a.hpos] = s_zero<S>();
                prog[j - 1] = 0;
            }
    }
    __syncthreads();
    // which 0: values in zl, right-hand side in place; which j >= 1: values in array j, rhs s * array j-1
    auto passes = [&](const int which) {
        const int lane = tid & 63, grp = lane >> 2, slot = lane & 3;
        const int nw = a.nwpass;
        S* zs = zl + which * pitch;
        const S* zp = zl + (which ? which - 1 : 0) * pitch;
        S rv[kWHeadDepth][4], rq[kWHeadDepth];
        int rc[kWHeadDepth][4], rd[kWHeadDepth];
        auto load = [&](int q, S* v, int* c, S& r, int& d) {
            const uint32_t qq = (uint32_t)(q < nw ? q : 0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t e = (qq * 4u + (uint32_t)k) * 64u + (uint32_t)lane;
                v[k] = ldg(a.wval, e);   // temporal loads: the head's data stays cached between solves
                c[k] = (int)ldg(a.wcol, e);
            }
            r = ldg(a.wrp, qq * (uint32_t)kWHeadRows + (uint32_t)grp);
            d = q < nw ? (int)ldg(a.wdst, qq * (uint32_t)kWHeadRows + (uint32_t)grp) : -1;
        };
#pragma unroll
        for (int u = 0; u < kWHeadDepth; ++u) load(u, rv[u], rc[u], rq[u], rd[u]);
        for (int q0 = 0; q0 < nw; q0 += kWHeadDepth) {
#pragma unroll
            for (int u = 0; u < kWHeadDepth; ++u) {   // straight line: nw is a multiple of the depth
                if (which) {
                    while (prog[which - 1] <= q0 + u) __builtin_amdgcn_s_sleep(1);
                    asm volatile("" ::: "memory");
                }
                S acc = mul(rv[u][0], zs[rc[u][0]]);
#pragma unroll
                for (int k = 1; k < 4; ++k) acc = add(acc, mul(rv[u][k], zs[rc[u][k]]));
                acc = quad_sum(acc);
                const int d = rd[u];
                if (slot == 0 && d >= 0) {
                    const S rhs = which ? scale_r(sanitize(zp[d]), s2) : zs[d];
                    zs[d] = mul(sub(rhs, acc), rq[u]);
                }
                asm volatile("" ::: "memory");   // this pass's store precedes the next pass's reads
                if (conc && which + 1 < K && lane == 0) prog[which] = q0 + u + 1;
                load(q0 + u + kWHeadDepth, rv[u], rc[u], rq[u], rd[u]);
            }
        }
    };
  for (int rep = 0; rep < K; ++rep) {
    if (!conc || rep == 0) {
        const int w = tid >> 6;
        if (w == 0 || (conc && w < K)) passes(w);
        __syncthreads();
    }
    // publish: the tail kernel (next in stream order) reads these through z
    S* zc = rep ? a.zk[rep] : a.zcur;
    S* zn = rep ? a.zkn[rep] : a.znext;
    S* yo = rep == K - 1 ? yout : a.aux[rep];
    const S* zsrc = zl + (conc ? rep : 0) * pitch;
    for (int p = tid; p < a.hpos; p += kWHeadThreads) {
        const int i = a.order[p];
        if (i < 0) continue;
        const S yi = sanitize(zsrc[p]);
        zc[i] = yi;
        yo[i] = yi;
        zn[i] = sentinel<S>();
        if (kMulti && !conc && rep + 1 < K) zl[p] = scale_r(yi, s2);   // the next solve's right-hand side
    }
    if (kMulti && !conc && rep + 1 < K) __syncthreads();
  }
}

// the chunk tails' back-off between re-polls of an unsolved value: pf = EIGSOL_TRSV_POLL_FAST in
// the low 16 bits (re-polls without a sleep), EIGSOL_TRSV_POLL_SLOW in bits 16-18 (the sleep
// schedule below, in units of 64 cycles: fewer re-poll requests against later wake-ups)
__device__ __forceinline__ void poll_backoff(int spins, int pf) {
    const int fast = pf & 0xffff, slow = pf >> 16;
    if (spins < fast) return;         // re-poll at once: the value is due within a round trip
    const int s = spins - fast;
    const int step = s < 4 ? 0 : (s < 16 ? 1 : 2);
    switch (slow * 3 + step) {        // s_sleep takes an immediate
        case 0: __builtin_amdgcn_s_sleep(2); break;     // 0: 2 / 8 / 32
        case 1: __builtin_amdgcn_s_sleep(8); break;
        case 2: __builtin_amdgcn_s_sleep(32); break;
        case 3: case 4: case 5: __builtin_amdgcn_s_sleep(4); break;       // 1: 4
        case 6: case 7: case 8: __builtin_amdgcn_s_sleep(6); break;       // 2: 6
        case 9: case 10: case 11: __builtin_amdgcn_s_sleep(16); break;    // 3: 16
        case 12: case 13: case 14: __builtin_amdgcn_s_sleep(8); break;    // 4: 8
        case 15: case 16: case 17: __builtin_amdgcn_s_sleep(32); break;   // 5: 32
        case 18: case 19: case 20: __builtin_amdgcn_s_sleep(12); break;   // 6: 12
        case 21: __builtin_amdgcn_s_sleep(16); break;   // 7: 16 / 24 / 32
        case 22: __builtin_amdgcn_s_sleep(24); break;
        default: __builtin_amdgcn_s_sleep(32); break;
    }
}

// first poll of a dependency is issued early (ld_coh); this finishes the wait
template <class S>
__device__ __forceinline__ S finish_wait(S y, const S* z, int j, int32_t* err, int pf) {
    int spins = 0;
    while (unready(y)) {
        poll_backoff(spins, pf);
        y = ld_cohi(z, j);
        if ((++spins & 255) == 0 && (spins > kSpinLimit || ld_flag_err(err) != 0)) {
            atomicOr(err, 1);
            break;
        }
    }
    return y;
}

// ---- tail: sync-free triangular solve over the remaining (wide) levels, one row per lane.
// The rows of each tail level are cut into slices of 64 (a level's last slice is padded with
// empty rows, so a slice never spans two levels and its lanes never wait on each other).  Slice
// s stores entry k of lane l at off_s + 64 k + l (coalesced), padded to at least B entries per
// lane with the zero slot z[n] (always 0) and value 0.  A lane computes its row exactly as the
// reference's back substitution does: s = b_i, s -= a_ij z_j in stored column order, y_i = s / d_i
// (oracle triu_shifted_solve_csr: bitwise equal when no FMA is contracted).
// Slices are dealt round-robin to the W waves, each taking its slices in increasing order.  A
// slice waits only on slices of strictly lower levels, i.e. earlier slices, so the earliest
// unfinished slice can always proceed provided every wave is resident: the kernel is launched
// cooperatively, so the runtime guarantees co-residency (or refuses the launch); a bounded spin
// plus a sticky error word still guarantee the grid drains.  (A ticket dispenser needs no
// co-residency, but 250k atomics on one word serialise: 3.3 ms against 0.9 ms.)
// Per slice: the B dependency loads (coherent; the solved value is its own ready flag, z starts
// as the sentinel NaN) and the B values are issued first, then the columns / row / pivot of the
// wave's next slice, so waiting on the dependencies does not wait on the prefetch (vmcnt retires
// in issue order).  Each launch resets the other z buffer row by row for the next launch (also
// when it exits early).  Norm / Rayleigh partials are reduced afterwards by shift_part_kernel.
template <class S, int B, bool kIter>
__global__ __launch_bounds__(kThreads) void sptrsv_slice_kernel(TriArgs<S> a, int parity) {
    __shared__ Prologue pro;
    const S* xin;
    S* yout;
    double nrm = 0.0;
    if constexpr (kIter) {
        shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) {
            // nothing to solve, but the next launch still expects its z reset
            for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * kThreads)
                a.znext[r] = sentinel<S>();
            return;
        }
        nrm = pro.nrm;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = gridDim.x * kWaves;
    const int ns = a.nslices;
    // consecutive slices (the slices of one level) go to consecutive workgroups, i.e. to
    // different CUs and XCDs, not to the four waves of one CU
    int s = wave * gridDim.x + blockIdx.x;

    int K, off, row;
    S piv;
    int col[B];
    auto fetch = [&](int s_, int& K_, int& off_, int* c, int& row_, S& piv_) {
        const bool in = s_ < ns;
        const int2 m = a.smeta[in ? s_ : 0];
        K_ = in ? m.y : 0;
        off_ = m.x;
#pragma unroll
        for (int k = 0; k < B; ++k) c[k] = (int)ldg_stream(a.tcol, (uint32_t)(off_ + 64 * k + lane));
        const uint32_t r = (uint32_t)((in ? s_ : 0) * 64 + lane);
        row_ = in ? (int)ldg_stream(a.trow, r) : -1;
        piv_ = ldg_stream(a.tpiv, r);
    };
    fetch(s, K, off, col, row, piv);
    for (; s < ns; s += W) {
        S z[B], v[B];
#pragma unroll
        for (int k = 0; k < B; ++k) z[k] = ld_cohi(a.zcur, col[k]);
#pragma unroll
        for (int k = 0; k < B; ++k) v[k] = ldg_stream(a.tval, (uint32_t)(off + 64 * k + lane));
        S bi = xin[row >= 0 ? row : 0];
        int Kn, offn, rown, coln[B];
        S pivn;
        fetch(s + W, Kn, offn, coln, rown, pivn);
        if constexpr (kIter) bi = scale_in(bi, nrm);
        S acc = bi;
        // dependencies not yet solved at the first load: poll them all together (one round trip
        // per poll round, not one per entry)
        bool pend = false;
#pragma unroll
        for (int k = 0; k < B; ++k) pend = pend || unready(z[k]);
        int spins = 0;
        while (pend) {
            if (spins >= (a.poll_fast & 0xffff)) {
                if (spins < (a.poll_fast & 0xffff) + 8) __builtin_amdgcn_s_sleep(2);
                else __builtin_amdgcn_s_sleep(16);
            }
            if (!(a.poll_mode & 1)) {
#pragma unroll
                for (int k = 0; k < B; ++k)
                    if (unready(z[k])) z[k] = ld_cohi(a.zcur, col[k]);
            } else {   // one poll per lane: its first unsolved dependency
                int kf = -1;
#pragma unroll
                for (int k = B - 1; k >= 0; --k)
                    if (unready(z[k])) kf = k;
                S zf = ld_cohi(a.zcur, kf >= 0 ? col[kf] : (int)a.n);
#pragma unroll
                for (int k = 0; k < B; ++k)
                    if (k == kf) z[k] = zf;
            }
            pend = false;
#pragma unroll
            for (int k = 0; k < B; ++k) pend = pend || unready(z[k]);
            if ((++spins & 255) == 0 && (spins > kSpinLimit || ld_flag_err(a.err) != 0)) {
                atomicOr(a.err, 1);
                break;
            }
        }
#pragma unroll
        for (int k = 0; k < B; ++k) acc = sub(acc, mul(v[k], z[k]));
        for (int k = B; k < K; ++k) {   // entries beyond B (long rows): one dependent round trip each
            const uint32_t e = (uint32_t)(off + 64 * k + lane);
            const int c = (int)a.tcol[e];
            acc = sub(acc, mul(a.tval[e], wait_value(a.zcur, c, a.err)));
        }
        if (row >= 0) {
            const S yi = sanitize(sdiv(acc, piv));
            st_cohi(a.zcur, row, yi);        // publish: readers poll this very word
            yout[row] = yi;
            a.znext[row] = sentinel<S>();
        }
        K = Kn;
        off = offn;
        row = rown;
        piv = pivn;
#pragma unroll
        for (int k = 0; k < B; ++k) col[k] = coln[k];
    }
}

// ---- tail, chunk variant: sync-free triangular solve, 16 lanes per row, 4 rows per chunk.
// Positions (level-ordered, every level padded to kWaveRows) form chunks of one wave round;
// chunk c belongs to wave (c - chunk0) mod W (consecutive chunks on consecutive workgroups), each
// wave taking its chunks in increasing order, two at a time: the dependency loads of a pair are
// issued at the end of the previous iteration (speculatively: a sentinel just means poll again),
// then the first chunk is solved and published, then the second (which may read the first).
// Progress needs every wave resident: launched cooperatively, like the slice variant.  Chosen
// for DAGs of many moderately wide levels (config 5: 0.86 ms against 1.3 ms for the slices,
// which wait on the slowest of 960 dependencies per wave); the slice variant wins on few, very
// wide levels (one 1M-row level: 74 us against 195 us).
template <class S>
struct RowMeta {
    int i, e0, len, j, j2;
    S v, v2, bi, pv;
};

// kTwo: rows of up to 2 x 16 entries (e.g. an LU factor with fill) keep a second entry per lane,
// whose dependency is polled together with the first instead of one round trip later
template <class S, bool kIter, bool kTwo = false>
__global__ __launch_bounds__(kThreads) void sptrsv_chunk_kernel(TriArgs<S> a, int parity) {
    __shared__ Prologue pro;
    const S* xin;
    S* yout;
    double nrm = 0.0;
    if constexpr (kIter) {
        shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) {
            for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * kThreads)
                a.znext[r] = sentinel<S>();
            return;
        }
        nrm = pro.nrm;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    const int tid = threadIdx.x;
    const int lane = tid & (kRowLanes - 1);
    const int grp = (tid & 63) / kRowLanes;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = gridDim.x * kWaves;
    const int gw = a.chunk0 + wave * gridDim.x + blockIdx.x;

    auto fetch1 = [&](int c, RowMeta<S>& m) {   // position-indexed metadata: no dependent loads
        const bool in = c < a.nchunks;
        const int pos = (in ? c : 0) * kWaveRows + grp;
        m.i = in ? a.porder[pos] : -1;
        const int e0 = a.pptr[pos];
        m.e0 = e0;
        m.len = in ? a.pptr[pos + 1] - e0 : 0;
        m.pv = ldg_stream(a.ppiv, (uint32_t)pos);
    };
    auto fetch2 = [&](RowMeta<S>& m) {         // the row's first 16 entries and its right side
        const bool ok = lane < m.len;
        const int e = ok ? m.e0 + lane : 0;
        m.j = ok ? (int)ldg_stream(a.pcol, (uint32_t)e) : -1;
        m.v = ldg_stream(a.pval, (uint32_t)e);
        if constexpr (kTwo) {
            const bool ok2 = lane + kRowLanes < m.len;
            const int e2 = ok2 ? m.e0 + lane + kRowLanes : 0;
            m.j2 = ok2 ? (int)ldg_stream(a.pcol, (uint32_t)e2) : -1;
            m.v2 = ldg_stream(a.pval, (uint32_t)e2);
        }
        m.bi = xin[m.i >= 0 ? m.i : 0];
    };
    auto solve = [&](const RowMeta<S>& m, S z0, S z0b) {
        S acc = s_zero<S>();
        if (m.j >= 0) acc = mul(m.v, finish_wait(z0, a.zcur, m.j, a.err, a.poll_fast));
        if constexpr (kTwo)
            if (m.j2 >= 0) acc = add(acc, mul(m.v2, finish_wait(z0b, a.zcur, m.j2, a.err, a.poll_fast)));
        for (int k = lane + (kTwo ? 2 : 1) * kRowLanes; k < m.len; k += kRowLanes) {   // rows longer than 16 / 32
            const int e = m.e0 + k;
            acc = add(acc, mul(a.pval[e], wait_value(a.zcur, a.pcol[e], a.err)));
        }
        acc = group_sum(acc);
        if (m.i >= 0 && lane == 0) {
            S bi = m.bi;
            if constexpr (kIter) bi = scale_in(bi, nrm);
            const S yi = sanitize(sdiv(sub(bi, acc), m.pv));
            st_cohi(a.zcur, m.i, yi);        // publish: readers poll this very word
            if constexpr (!kIter) {          // iteration: shift_part_kernel<S, true> moves y out
                yout[m.i] = yi;
                a.znext[m.i] = sentinel<S>();
            }
        }
    };

    RowMeta<S> c0, c1, n0, n1;
    fetch1(gw, c0);
    fetch1(gw + W, c1);
    fetch2(c0);
    fetch2(c1);
    fetch1(gw + 2 * W, n0);
    fetch1(gw + 3 * W, n1);
    // EIGSOL_TRSV_POLL_MODE bit 1: the second chunk's first polls after the first chunk is solved
    const int late = a.poll_mode & 2;
    auto first_poll = [&](int j) { return j >= 0 ? ld_cohi(a.zcur, j) : s_zero<S>(); };
    S z0 = first_poll(c0.j), z1 = first_poll(c1.j);
    S z0b = s_zero<S>(), z1b = s_zero<S>();
    if constexpr (kTwo) {
        z0b = first_poll(c0.j2);
        z1b = first_poll(c1.j2);
    }
    for (int c = gw; c < a.nchunks; c += 2 * W) {
        fetch2(n0);
        fetch2(n1);
        RowMeta<S> m0, m1;
        fetch1(c + 4 * W, m0);
        fetch1(c + 5 * W, m1);
        solve(c0, z0, z0b);
        if (late) {
            z1 = first_poll(c1.j);
            if constexpr (kTwo) z1b = first_poll(c1.j2);
        }
        solve(c1, z1, z1b);
        z0 = first_poll(n0.j);
        if constexpr (kTwo) z0b = first_poll(n0.j2);
        if (!late) {
            z1 = first_poll(n1.j);
            if constexpr (kTwo) z1b = first_poll(n1.j2);
        }
        c0 = n0;
        c1 = n1;
        n0 = m0;
        n1 = m1;
    }
}

// ---- tail of a multi-solve launch (shift_multi_prologue), role split: the grid is K copies of
// the single-solve grid.  Blocks [jG, (j+1)G) run sptrsv_chunk_kernel's schedule for solve j:
// w_0 = (A - sigma I)^{-1} x, w_j = (A - sigma I)^{-1} (s w_{j-1}), taking each row's right-hand
// side s (w_{j-1})_i from solve j-1's polled value (its ready flag) and their dependencies from
// zk[j].  A wave waits only on its own solve's chains (and on the row of the solve before), so
// solve j trails solve j-1 by about one dependency round trip.  The matrix is read once per
// solve.  No deadlock: solve j-1 never waits on solve j, and every wave is resident (cooperative
// launch).  Measured on config 5 (pair launches, K = 2): 0.539 ms per iteration at one workgroup
// per CU per solve against 0.555 at two, and 0.58 ms for an interleaved schedule (each wave
// solving its chunks of round r for w_0, then those of round r - 1 for w_1: a wave's second-solve
// waits then add to its first-solve waits).
template <class S>
__global__ __launch_bounds__(kThreads) void sptrsv_chunk_role_kernel(TriArgs<S> a, int parity) {
    __shared__ Prologue pro;
    shift_multi_prologue<S>(a.ctl, a.rank_part, a.kpart, a.K, parity, a.trace, a.sig_re, a.sig_im, &pro);
    if (!__builtin_amdgcn_readfirstlane(pro.go)) {
        for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * kThreads)
            for (int j = 0; j < a.K; ++j) a.zkn[j][r] = sentinel<S>();
        return;
    }
    const int G = (int)gridDim.x / a.K;
    const int role = __builtin_amdgcn_readfirstlane((int)blockIdx.x / G);
    const int blk = (int)blockIdx.x - role * G;
    const double nrm = pro.nrm, s2 = pro.s;
    const S* xin = parity ? a.buf0 : a.buf1;
    S* zdep = a.zk[role];                          // dependencies and publication
    const S* zrhs = a.zk[role ? role - 1 : 0];     // solve j >= 1: the previous solve's values
    const int tid = threadIdx.x;
    const int lane = tid & (kRowLanes - 1);
    const int grp = (tid & 63) / kRowLanes;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = G * kWaves;
    const int gw = a.chunk0 + wave * G + blk;

    auto fetch1 = [&](int c, RowMeta<S>& m) {
        const bool in = c < a.nchunks;
        const int pos = (in ? c : 0) * kWaveRows + grp;
        m.i = in ? a.porder[pos] : -1;
        const int e0 = a.pptr[pos];
        m.e0 = e0;
        m.len = in ? a.pptr[pos + 1] - e0 : 0;
        m.pv = ldg_stream(a.ppiv, (uint32_t)pos);
    };
    auto fetch2 = [&](RowMeta<S>& m) {
        const bool ok = lane < m.len;
        const int e = ok ? m.e0 + lane : 0;
        m.j = ok ? (int)ldg_stream(a.pcol, (uint32_t)e) : -1;
        m.v = ldg_stream(a.pval, (uint32_t)e);
        // second solve: the first solve's value of the row, possibly not yet solved (polled below)
        m.bi = role ? ld_cohi(zrhs, (m.i >= 0 ? m.i : (int)a.n)) : xin[m.i >= 0 ? m.i : 0];
    };
    auto solve = [&](const RowMeta<S>& m, S z0) {
        S acc = s_zero<S>();
        S bv = m.bi;
        if (role) {
            // the dependency and (lane 0) the first solve's value of the row are polled in the same
            // loop: waiting for them one after the other would add a round trip to every level
            const bool nb = lane == 0 && m.i >= 0;
            S zv = m.j >= 0 ? z0 : s_zero<S>();
            int spins = 0;
            while (unready(zv) || (nb && unready(bv))) {
                poll_backoff(spins, a.poll_fast & ~0xffff);
                if (unready(zv)) zv = ld_cohi(zdep, m.j);
                if (nb && unready(bv)) bv = ld_cohi(zrhs, m.i);
                if ((++spins & 255) == 0 && (spins > kSpinLimit || ld_flag_err(a.err) != 0)) {
                    atomicOr(a.err, 1);
                    break;
                }
            }
            if (m.j >= 0) acc = mul(m.v, zv);
        } else if (m.j >= 0) {
            acc = mul(m.v, finish_wait(z0, zdep, m.j, a.err, a.poll_fast));
        }
        for (int k = lane + kRowLanes; k < m.len; k += kRowLanes) {
            const int e = m.e0 + k;
            acc = add(acc, mul(a.pval[e], wait_value(zdep, a.pcol[e], a.err)));
        }
        acc = group_sum(acc);
        if (m.i >= 0 && lane == 0) {
            S bi;
            if (role) bi = scale_r(bv, s2);
            else bi = scale_in(m.bi, nrm);
            const S yi = sanitize(sdiv(sub(bi, acc), m.pv));
            st_cohi(zdep, m.i, yi);        // moved out by shift_multi_part_kernel
        }
    };

    RowMeta<S> c0, c1, n0, n1;
    fetch1(gw, c0);
    fetch1(gw + W, c1);
    fetch2(c0);
    fetch2(c1);
    fetch1(gw + 2 * W, n0);
    fetch1(gw + 3 * W, n1);
    // EIGSOL_TRSV_POLL_MODE bit 1: the second chunk's first polls are issued after the first
    // chunk is solved instead of a round ahead (fewer polls of still-unsolved values); bit 2: both
    // chunks' first polls at the top of the round
    const int late = a.poll_mode;
    S z0 = c0.j >= 0 ? ld_cohi(zdep, c0.j) : s_zero<S>();
    S z1 = c1.j >= 0 ? ld_cohi(zdep, c1.j) : s_zero<S>();
    for (int c = gw; c < a.nchunks; c += 2 * W) {
        if (late & 4) {
            z0 = c0.j >= 0 ? ld_cohi(zdep, c0.j) : s_zero<S>();
            z1 = c1.j >= 0 ? ld_cohi(zdep, c1.j) : s_zero<S>();
        }
        fetch2(n0);
        fetch2(n1);
        RowMeta<S> m0, m1;
        fetch1(c + 4 * W, m0);
        fetch1(c + 5 * W, m1);
        solve(c0, z0);
        if (late & 2) z1 = c1.j >= 0 ? ld_cohi(zdep, c1.j) : s_zero<S>();
        solve(c1, z1);
        if (!(late & 4)) z0 = n0.j >= 0 ? ld_cohi(zdep, n0.j) : s_zero<S>();
        if (!(late & 6)) z1 = n1.j >= 0 ? ld_cohi(zdep, n1.j) : s_zero<S>();
        c0 = n0;
        c1 = n1;
        n0 = m0;
        n1 = m1;
    }
}

// Partials of a multi-solve launch, solve j: {||w_j||^2, w_{j-1}^H w_j} (w_{-1} = x) -> my_part
// (j = 0) or kpart[j - 1], each in a fixed order (grid-stride per thread, block sums, last-arriver
// sum in block order).  The solves left w_j only in their polled buffers: this kernel moves them
// out (aux[j], the last one to B[parity]) and resets the next launch's buffers, in coalesced
// streams.
template <class S>
__global__ __launch_bounds__(kThreads) void shift_multi_part_kernel(TriArgs<S> a, int parity) {
    __shared__ double sm[3 * kWaves];
    __shared__ int s_last[kMaxMulti];
    __shared__ int s_go;
    __shared__ double s_nrm;
    if (threadIdx.x == 0) {
        s_go = __hip_atomic_load(&a.ctl->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
        s_nrm = a.ctl->st[parity ^ 1].nrm;
    }
    __syncthreads();
    if (!s_go) return;
    const double nrm = s_nrm;
    const int K = a.K;
    const S* xin = parity ? a.buf0 : a.buf1;
    S* wlast = parity ? a.buf1 : a.buf0;
    double n2[kMaxMulti] = {}, dr[kMaxMulti] = {}, di[kMaxMulti] = {};
#pragma unroll 2
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        S prev = scale_in(xin[i], nrm);
#pragma unroll
        for (int j = 0; j < kMaxMulti; ++j) {
            if (j < K) {
                const S y = a.zk[j][i];
                (j == K - 1 ? wlast : a.aux[j])[i] = y;
                a.zkn[j][i] = sentinel<S>();
                n2[j] += sq_abs(y);
                acc_dot(dr[j], di[j], prev, y);
                prev = y;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxMulti; ++j) {
        if (j < K) {
            block_sum3(n2[j], dr[j], di[j], sm);
            last_arriver_reduce(n2[j], dr[j], di[j], j ? a.kblk + (size_t)(j - 1) * gridDim.x : a.wave_part,
                                a.work + 2 + j, j ? a.kpart + (j - 1) : a.my_part, sm, &s_last[j]);
        }
    }
}

// GMRES path: the launch prologue alone (the stop decision and ||y_{t-1}||), the solve follows on
// the host's word
template <class S>
__global__ __launch_bounds__(64) void shift_decide_kernel(TriArgs<S> a, int parity) {
    __shared__ Prologue pro;
    shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
}

// Norm and Rayleigh partials of a solved iterate, in a fixed order (grid-stride per thread,
// block sums, last-arriver sum in block order): sum |y_i|^2 and sum conj(x_i) y_i with
// x = b / ||y_prev|| as the solve used it.  Skipped once the prologue has stopped the loop.
// kFromZ (triangular factors): the solve left y only in the polled buffer zcur; this kernel also
// moves it to B[parity] and resets znext to the sentinel for the next launch (coalesced streams,
// instead of two scattered 16-byte stores per row inside the latency-bound solve)
template <class S, bool kFromZ = false>
__global__ __launch_bounds__(kThreads) void shift_part_kernel(TriArgs<S> a, int parity) {
    __shared__ double sm[3 * kWaves];
    __shared__ int s_last;
    __shared__ int s_go;
    __shared__ double s_nrm;
    if (threadIdx.x == 0) {
        s_go = __hip_atomic_load(&a.ctl->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
        s_nrm = a.ctl->st[parity ^ 1].nrm;
    }
    __syncthreads();
    if (!s_go) return;
    const double nrm = s_nrm;
    const S* xin = parity ? a.buf0 : a.buf1;
    S* y = parity ? a.buf1 : a.buf0;
    double n2 = 0.0, pr = 0.0, pi = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        S yi;
        if constexpr (kFromZ) {
            yi = a.zcur[i];
            y[i] = yi;
            a.znext[i] = sentinel<S>();
        } else {
            yi = y[i];
        }
        n2 += sq_abs(yi);
        acc_dot(pr, pi, scale_in(xin[i], nrm), yi);   // p = sum conj(x_i) y_i
    }
    block_sum3(n2, pr, pi, sm);
    last_arriver_reduce(n2, pr, pi, a.wave_part, a.work + 2, a.my_part, sm, &s_last);
}

}  // namespace dev

template <class S>
static const void* slice_kernel_ptr(int b, bool iter) {
    if (b == 4) return iter ? reinterpret_cast<const void*>(dev::sptrsv_slice_kernel<S, 4, true>)
                            : reinterpret_cast<const void*>(dev::sptrsv_slice_kernel<S, 4, false>);
    if (b == 8) return iter ? reinterpret_cast<const void*>(dev::sptrsv_slice_kernel<S, 8, true>)
                            : reinterpret_cast<const void*>(dev::sptrsv_slice_kernel<S, 8, false>);
    return iter ? reinterpret_cast<const void*>(dev::sptrsv_slice_kernel<S, 16, true>)
                : reinterpret_cast<const void*>(dev::sptrsv_slice_kernel<S, 16, false>);
}

// Launch geometry of a level-ordered triangular factor (host- or device-built): the tail grid (one
// residency round, cooperative launch), the multi-solve set-up and the partials grid.  Needs the
// layout fields (tail variant, chunk_two, slice_b, head, chunks / slices) already set.
template <class S>
static int tri_launch_setup_t(ShiftFactor* f) {
    int rc = EIGSOL_OK;
    // tail grid: one residency round (cooperative launch), capped at kTrsvBlocksPerCU
    // blocks per CU and by the work
    {
        int per_cu_max = 0;
        const void* tk = f->tri.tail_chunks ? (f->tri.chunk_two ? reinterpret_cast<const void*>(dev::sptrsv_chunk_kernel<S, true, true>)
                                                        : reinterpret_cast<const void*>(dev::sptrsv_chunk_kernel<S, true>))
                                        : slice_kernel_ptr<S>(f->tri.slice_b, true);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_max, tk, dev::kThreads, 0) != hipSuccess ||
            per_cu_max < 1)
            rc = fail(EIGSOL_E_HIP, "triangular solve: occupancy query");
        f->tri.grid = per_cu_max * f->ctx->num_cus;
    }
    constexpr int kTrsvBlocksPerCU = 2;
    f->tri.grid = std::min(f->tri.grid, kTrsvBlocksPerCU * f->ctx->num_cus);
    const int64_t units = f->tri.tail_chunks ? (int64_t)f->tri.nchunks - f->tri.chunk0 : f->tri.nslices;
    f->tri.grid = (int)std::max<int64_t>(1, std::min<int64_t>(f->tri.grid, (units + dev::kWaves - 1) / dev::kWaves));
    // multi-solve launches: chunk tail with the one-wave head (or none), K solves per launch
    // (EIGSOL_TRSV_MULTI=K, 1..4; 1 = one iteration per launch) on K copies of the grid at one
    // workgroup per CU per solve, when they are co-resident
    if (rc == EIGSOL_OK && f->tri.tail_chunks && (f->tri.hpos == 0 || f->tri.wave_head)) {
        const char* e = std::getenv("EIGSOL_TRSV_MULTI");
        const int want = std::max(1, std::min(dev::kMaxMulti, e ? std::atoi(e) : kMultiDefault));
        int per_cu_role = 0;
        hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu_role, reinterpret_cast<const void*>(dev::sptrsv_chunk_role_kernel<S>), dev::kThreads, 0);
        const int gr = std::min(f->tri.grid, f->ctx->num_cus);   // one role block per CU
        int K = want;
        while (K > 1 && per_cu_role * f->ctx->num_cus < K * gr) --K;
        if (K > 1) {
            f->tri.multi = K;
            f->tri.grid_multi = K * gr;
            const char* hc = std::getenv("EIGSOL_TRSV_MULTI_HEAD");   // seq: the head solves one after another
            // the dynamic LDS of the concurrent head shares the CU's 160 KiB with the kernel's static
            // __shared__ state (its prologue record)
            hipFuncAttributes fa{};
            size_t static_lds = 256;
            if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(dev::sptrsv_whead_kernel<S, true, true>)) ==
                hipSuccess)
                static_lds = fa.sharedSizeBytes;
            f->tri.hconc = (!(hc && !std::strcmp(hc, "seq")) &&
                        (size_t)K * (size_t)(f->tri.hpos + 1) * sizeof(S) + 16 + static_lds <= (size_t)160 * 1024) ? 1 : 0;
        }
    }
    // the partials kernels' grid.  Round 6 (profiles/r06_c5_partgrid_ab.log, config 5 at K = 4): 2048 / 977 (n / 1024, the old cap) / 512 /
    // 256 / 192 / 128 / 64 blocks -> 0.4077 / 0.4076 / 0.4026 / 0.4010 / 0.4016 / 0.4049 / 0.4159 ms per
    // iteration: one block per CU, the last arriver sums fewer block partials per solve
    constexpr int64_t red_cap = 256;
    // never above grid * kWaves: wave_part (below) holds that many block partials
    f->tri.red_grid = (int)std::max<int64_t>(1, std::min<int64_t>(f->tri.grid * dev::kWaves,
                                                                  std::min<int64_t>(red_cap, (f->n + 1023) / 1024)));
    return rc;
}

int tri_launch_setup(ShiftFactor* f) {
    return by_dtype(f->dtype, [&](auto tag) { return tri_launch_setup_t<decltype(tag)>(f); });
}

// buffers of the multi-solve launches, allocated by the first iteration launch (plain solves, e.g. the
// GMRES path's ILU(0) factors, never need them)
template <class S>
static int multi_alloc(ShiftFactor* f) {
    if (f->tri.kpart) return EIGSOL_OK;
    hipStream_t st = f->ctx->stream;
    const int64_t n = f->n;
    const int K = f->tri.multi;
    // buffer by buffer, so that a call after a failed allocation resumes instead of leaking
    for (int j = 0; j + 1 < K; ++j)
        if (!f->tri.aux[j]) EIGSOL_HIP(hipMalloc(&f->tri.aux[j], (size_t)std::max<int64_t>(n, 1) * sizeof(S)));
    for (int j = 1; j < K; ++j)
        for (void*& zb : f->tri.zm[j]) {
            if (zb) continue;
            EIGSOL_HIP(hipMalloc(&zb, (size_t)(n + 1) * sizeof(S)));
            const uint32_t sent = (uint32_t)(dev::kSent & 0xffffffffu);
            EIGSOL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(zb), (int)sent, n * sizeof(S) / 4, st));
            EIGSOL_HIP(hipMemsetAsync(static_cast<char*>(zb) + n * sizeof(S), 0, sizeof(S), st));
        }
    if (!f->tri.kblk) EIGSOL_HIP(hipMalloc(&f->tri.kblk, (size_t)(K - 1) * std::max(1, f->tri.red_grid) * sizeof(dev::part4)));
    EIGSOL_HIP(hipMalloc(&f->tri.kpart, (size_t)(K - 1) * sizeof(dev::part4)));   // last: marks the set complete
    EIGSOL_HIP(hipMemsetAsync(f->tri.kpart, 0, (size_t)(K - 1) * sizeof(dev::part4), st));
    return EIGSOL_OK;
}

// the final iterate of a multi-solve launch that stopped on solve j < K - 1 (final_parity 2 + j)
void* shift_aux(const ShiftFactor* f, int j) { return (j >= 0 && j < dev::kMaxMulti - 1) ? f->tri.aux[j] : nullptr; }

// One solve, or one iteration launch: the head kernel (levels too narrow for the tail), the cooperative tail, and
// in iteration mode the partials reduction.
template <class S>
static int tri_launch_t(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it, bool first) {
    hipStream_t st = f->ctx->stream;
    TriFactor& t = f->tri;
    int parity = it.parity;
    dev::TriArgs<S> a{};
    fill_iter(a, f, b, y, it);
    a.order = t.order;
    const int e = ++t.epoch;
    a.zcur = static_cast<S*>(t.z[e & 1]);
    a.znext = static_cast<S*>(t.z[(e + 1) & 1]);
    a.work = t.work;
    a.err = t.err;
    a.wave_part = static_cast<dev::part4*>(t.wave_part);
    a.hcol = t.hcol;
    a.hval = static_cast<const S*>(t.hval);
    a.hpiv = static_cast<const S*>(t.hpiv);
    a.passes = t.passes;
    a.npass = t.npass;
    a.hpos = t.hpos;
    a.poll_fast = t.poll_fast;
    a.poll_mode = t.poll_mode;
    a.wval = static_cast<const S*>(t.wval);
    a.wcol = t.wcol;
    a.wrp = static_cast<const S*>(t.wrp);
    a.wdst = t.wdst;
    a.nwpass = t.nwpass;
    // multi-solve launch; a session's launch 0 is a single solve (it measures the growth that
    // scales the chained solves of the later launches, shift_multi_prologue)
    const bool pair = iter && t.multi > 1 && !first;
    a.K = 1;
    a.zk[0] = a.zcur;
    a.zkn[0] = a.znext;
    if (pair) {
        EIGSOL_TRY(multi_alloc<S>(f));
        const int em = ++t.epoch_m;   // its own epoch: plain solves in between never skip a reset
        a.K = t.multi;
        for (int j = 1; j < t.multi; ++j) {
            a.zk[j] = static_cast<S*>(t.zm[j][em & 1]);
            a.zkn[j] = static_cast<S*>(t.zm[j][(em + 1) & 1]);
        }
        for (int j = 0; j + 1 < t.multi; ++j) a.aux[j] = static_cast<S*>(t.aux[j]);
        a.kpart = static_cast<dev::part4*>(t.kpart);
        a.kblk = static_cast<dev::part4*>(t.kblk);
    }
    if (t.hpos > 0 && t.wave_head && pair) {
        a.hconc = t.hconc;
        const size_t wl = (size_t)(t.hpos + 1) * sizeof(S) * (t.hconc ? t.multi : 1) + (t.hconc ? 16 : 0);
        const void* hk = reinterpret_cast<const void*>(dev::sptrsv_whead_kernel<S, true, true>);
        EIGSOL_HIP(hipFuncSetAttribute(hk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wl));
        hipLaunchKernelGGL((dev::sptrsv_whead_kernel<S, true, true>), dim3(1), dim3(dev::kWHeadThreads), wl, st, a,
                           parity);
    } else if (t.hpos > 0 && t.wave_head) {
        const size_t wl = (size_t)(t.hpos + 1) * sizeof(S);
        const void* hk = iter ? reinterpret_cast<const void*>(dev::sptrsv_whead_kernel<S, true>)
                              : reinterpret_cast<const void*>(dev::sptrsv_whead_kernel<S, false>);
        EIGSOL_HIP(hipFuncSetAttribute(hk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wl));
        if (iter) hipLaunchKernelGGL((dev::sptrsv_whead_kernel<S, true>), dim3(1), dim3(dev::kWHeadThreads), wl, st, a, parity);
        else hipLaunchKernelGGL((dev::sptrsv_whead_kernel<S, false>), dim3(1), dim3(dev::kWHeadThreads), wl, st, a, parity);
    }
    const size_t hl = (size_t)(t.hpos + 1) * sizeof(S) + (size_t)t.npass * sizeof(int2);
    if (t.hpos > 0 && !t.wave_head) {
        const void* hk = iter ? reinterpret_cast<const void*>(dev::sptrsv_head_kernel<S, true>)
                              : reinterpret_cast<const void*>(dev::sptrsv_head_kernel<S, false>);
        EIGSOL_HIP(hipFuncSetAttribute(hk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hl));
        if (iter) hipLaunchKernelGGL((dev::sptrsv_head_kernel<S, true>), dim3(1), dim3(dev::kHeadThreads), hl, st, a, parity);
        else hipLaunchKernelGGL((dev::sptrsv_head_kernel<S, false>), dim3(1), dim3(dev::kHeadThreads), hl, st, a, parity);
    }
    // a head that failed to launch would leave the tail polling for values nobody writes
    EIGSOL_HIP(hipGetLastError());
    // cooperative: the static chunk schedule needs every wave of the grid resident
    void* kargs[] = {&a, &parity};
    a.smeta = t.smeta;
    a.trow = t.trow;
    a.tpiv = static_cast<const S*>(t.tpiv);
    a.tcol = t.tcol;
    a.tval = static_cast<const S*>(t.tval);
    a.nslices = t.nslices;
    a.porder = t.porder;
    a.pptr = t.pptr;
    a.pcol = t.pcol;
    a.pval = static_cast<const S*>(t.pval);
    a.ppiv = static_cast<const S*>(t.ppiv);
    a.chunk0 = t.chunk0;
    a.nchunks = t.nchunks;
    const void* tk = pair ? reinterpret_cast<const void*>(dev::sptrsv_chunk_role_kernel<S>)
                     : !t.tail_chunks ? slice_kernel_ptr<S>(t.slice_b, iter)
                     : t.chunk_two ? (iter ? reinterpret_cast<const void*>(dev::sptrsv_chunk_kernel<S, true, true>)
                                            : reinterpret_cast<const void*>(dev::sptrsv_chunk_kernel<S, false, true>))
                     : iter ? reinterpret_cast<const void*>(dev::sptrsv_chunk_kernel<S, true>)
                            : reinterpret_cast<const void*>(dev::sptrsv_chunk_kernel<S, false>);
    const int tgrid = pair ? t.grid_multi : t.grid;
    // EIGSOL_TRSV_NO_COOP=1: the same kernel through an ordinary launch, for profiling only
    // (rocprofv3 7.2 segfaults in its exit-time finaliser after any cooperative launch,
    // tools/coop_prof_repro.hip); the grid is one residency round, so on an otherwise idle
    // device every wave is resident anyway
    static const bool no_coop = std::getenv("EIGSOL_TRSV_NO_COOP") != nullptr;
    if (no_coop) EIGSOL_HIP(hipLaunchKernel(tk, dim3(tgrid), dim3(dev::kThreads), kargs, 0, st));
    else EIGSOL_HIP(hipLaunchCooperativeKernel(tk, dim3(tgrid), dim3(dev::kThreads), kargs, 0, st));
    if (pair)
        hipLaunchKernelGGL((dev::shift_multi_part_kernel<S>), dim3(t.red_grid), dim3(dev::kThreads), 0, st, a,
                           parity);
    else if (iter)   // every tail kernel publishes y in zcur (the chunk tail only there)
        hipLaunchKernelGGL((dev::shift_part_kernel<S, true>), dim3(t.red_grid), dim3(dev::kThreads), 0, st, a,
                           parity);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

int tri_launch(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it, bool first) {
    return by_dtype(f->dtype, [&](auto tag) { return tri_launch_t<decltype(tag)>(f, iter, b, y, it, first); });
}

// The GMRES family's iteration (shifted.hip) is host-driven: shift_decide_kernel takes the launch's stop decision
// for the host to read, shift_part_kernel reduces the partials of the iterate the host-driven solve left in B.
template <class S>
static dev::TriArgs<S> gmres_iter_args(const ShiftFactor* f, const ShiftIter& it) {
    dev::TriArgs<S> a{};
    fill_iter(a, f, nullptr, nullptr, it);
    a.work = f->gmres.work;
    a.wave_part = static_cast<dev::part4*>(f->gmres.wave_part);
    return a;
}

int iter_decide_launch(ShiftFactor* f, const ShiftIter& it) {
    return by_dtype(f->dtype, [&](auto tag) -> int {
        using S = decltype(tag);
        hipLaunchKernelGGL((dev::shift_decide_kernel<S>), dim3(1), dim3(64), 0, f->ctx->stream, gmres_iter_args<S>(f, it),
                           it.parity);
        return EIGSOL_OK;
    });
}

int iter_part_launch(ShiftFactor* f, const ShiftIter& it) {
    return by_dtype(f->dtype, [&](auto tag) -> int {
        using S = decltype(tag);
        hipLaunchKernelGGL((dev::shift_part_kernel<S>), dim3(f->gmres.red_grid), dim3(dev::kThreads), 0, f->ctx->stream,
                           gmres_iter_args<S>(f, it), it.parity);
        EIGSOL_HIP(hipGetLastError());
        return EIGSOL_OK;
    });
}

}  // namespace eigsol
