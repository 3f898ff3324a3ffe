// The host half of the multifrontal LU (multifrontal_plan.cpp): ordering, symbolic structure, launch
// and solve tables.  Plain C++ - no device header - so the plan builds and runs without a device;
// multifrontal.hip uploads these tables and owns every kernel that reads them.
#pragma once

#include <atomic>
#include <cstdint>
#include <vector>

#include "multifrontal.hpp"

namespace eigsol {

// panel width of the numeric factorization per scalar type: RankKMax<double> / RankKMax<cplx> of
// mfma_rankk.hpp (a device header; multifrontal.hip asserts the equality)
constexpr int kMfPanelF64 = 64, kMfPanelC128 = 32;

namespace dev {

struct MfFront {
    int64_t off;    // front at F + off: d x d, column-major, leading dimension d
    int64_t uoff;   // forward contribution vector (ms entries) at u + uoff
    int64_t sof;    // struct indices (new numbering) at sidx + sof; their positions in the parent's list at cmap + sof
    int32_t d, ns, c0, ms;
    int32_t ch0, ch1;   // children chl[ch0 .. ch1) (fixed order)
    int32_t parent;
    int32_t flag0;  // large fronts: first of the front's pivot-block flags; -1: solved by one workgroup
    int64_t zoff;   // large fronts: assembled right-hand side (d entries) at z + zoff
    int64_t goff;   // inverse form (ns <= 64, d <= 256; -1: none) at F + goff: [inv(L11); L21 inv(L11)]
                    // (d x ns, ld d), then [inv(U11), -inv(U11) U12] (ns x d, ld ns)
};

}  // namespace dev

// The ordering and symbolic structure (host only): fronts in postorder with their columns,
// structs, children, parent maps; per-height lists; work and size figures.
struct MfPlan {
    int64_t nt = 0;
    std::vector<int32_t> perm, iperm, snode, chl, sidx, cmap, height, lists;
    std::vector<int64_t> sof, hstart;
    std::vector<dev::MfFront> fr;
    int32_t H = 0;
    int64_t maxd = 0, maxns = 0, uo = 0;
    double fe = 0.0, fac = 0.0, flops = 0.0;
};

// returns false on an internal inconsistency (a struct entry outside the ancestors)
// max_front_entries: the plan is abandoned once the fronts' sum of d^2 passes it (a pattern
// without small separators, e.g. a random graph); stop: abandoned when raised (another thread's
// factor won)
bool mf_plan(int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int leaf, bool cplx_flops,
             MfPlan& P, double max_front_entries = 1e300, const std::atomic<bool>* stop = nullptr);

struct MfLaunch {
    int kind;   // 0 extend, 1 panel, 2 gemm
    int32_t h, q;
    int64_t off, cnt;
};

// What the solve needs per height h: the one-workgroup fronts (slists[sstart[h] .. + nsmall[h])),
// then the large fronts (the next nbig[h] entries: their assembly launch); the large fronts'
// row-block tables (front, block) for the forward / backward launches at tabf / tabb + 2 off[h],
// cnt[h] pairs; dynamic LDS bytes of the height's launches.
struct MfSolveTables {
    std::vector<int64_t> sstart, nsmall, nbig, foff, fcnt, boff, bcnt;
    std::vector<int32_t> lds_fwd, lds_bwd;   // one-workgroup fronts (mf_fwd_kernel / mf_bwd_kernel)
    std::vector<int32_t> lds_bbig;           // x(struct) of the large fronts (mf_big_bwd_kernel)
    std::vector<int32_t> lds_asm;            // mf_big_asm_kernel: ns entries per large front
    std::vector<int32_t> lds_asm2;           // mf_fwd_height_kernel's assembly: d entries per large front
};

struct MfHost {
    MfPlan P;
    int64_t n = 0, nnz = 0;
    int nb = 32;
    int64_t sb = 16;
    std::vector<int64_t> dst;              // M's entries -> front offsets
    std::vector<MfLaunch> plan;            // factorization launches
    std::vector<int32_t> tab, slists, tabf, tabb;
    MfSolveTables T;
    int32_t nflag = 0;
    int64_t zsz = 0;
    std::vector<int32_t> inv_list;         // fronts with an inverse form (MfFront::goff)
    int64_t gsz = 0;                       // its scalars, stored after the fronts in F
    MfStats stt;
};

}  // namespace eigsol
