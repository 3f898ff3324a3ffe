// Host program for the multifrontal plan (csrc/multifrontal_plan.cpp), for tests/test_mf_plan_host_cpu.py.
// Plain C++, linked with multifrontal_plan.cpp only: no HIP runtime, no device.
//
// It builds its patterns itself (tests/test_mf_plan_host_cpu.py builds the same ones for eigsol_mf_analyze):
//   grid NX   the 5-point grid, NX x NX, natural order, diagonal stored
//   comps     grid 20, seven empty rows, grid 15 on the diagonal; row 3 gets 80 further distinct columns
//   band      n = 500: 3000 draws (r, clip(r + k - 30, 0, n - 1)), k in [0, 35), duplicates merged
// (random draws: x <- 6364136223846793005 x + 1442695040888963407 mod 2^64 from the seed, value x >> 33)
// and runs mf_prepare on each for EIGSOL_F64 and EIGSOL_C128 with EIGSOL_MF_LEAF / EIGSOL_MF_THREADS set by
// setenv.  One line per run:
//   case NAME DTYPE STATUS fronts heights max_front max_pivots factor_entries front_entries flops ok HPERM HFRONTS
// HPERM / HFRONTS: h <- (h ^ (uint32) word) * 1099511628211 mod 2^64 from 14695981039346656037 over perm and over
// the fronts' (c0, ns, ms, parent); "ok" is 1 for status 0.  The cancellation runs (grid 160, one host thread)
// print "cancel NAME DTYPE STATUS": "late" raises *stop from a second thread about 1 ms into the plan, "early"
// has it set on entry; both must give EIGSOL_E_UNSUPPORTED (12).  A last "case" line repeats grid 160 afterwards.
//
// Sanitizer builds, run by hand on the host (never under pytest, never on a device machine), from the repository
// root with CXX the ROCm clang++ and SRC="tests/cpp/mf_plan_host.cpp pcsc_eigenvalue_solver_project_amd/csrc/multifrontal_plan.cpp",
// INC="-Iinclude -Ipcsc_eigenvalue_solver_project_amd/csrc" (each one command line):
//   $CXX -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined $INC $SRC -pthread -o mf_plan_host_asan && ./mf_plan_host_asan
//   $CXX -std=c++17 -O1 -g -fsanitize=thread $INC $SRC -pthread -o mf_plan_host_tsan && ./mf_plan_host_tsan
// Both ran every case clean (no report, the same 24 lines as the plain build) when this file was written.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "multifrontal_plan.hpp"

using namespace eigsol;

namespace {

struct Pattern {
    int64_t n = 0;
    std::vector<int32_t> rp, ci;
};

Pattern from_rows(const std::vector<std::set<int32_t>>& rows) {
    Pattern p;
    p.n = (int64_t)rows.size();
    p.rp.push_back(0);
    for (const auto& r : rows) {
        p.ci.insert(p.ci.end(), r.begin(), r.end());
        p.rp.push_back((int32_t)p.ci.size());
    }
    return p;
}

void add_grid(std::vector<std::set<int32_t>>& rows, int nx, int32_t base) {
    for (int y = 0; y < nx; ++y)
        for (int x = 0; x < nx; ++x) {
            auto& r = rows[base + y * nx + x];
            r.insert(base + y * nx + x);
            if (x > 0) r.insert(base + y * nx + x - 1);
            if (x + 1 < nx) r.insert(base + y * nx + x + 1);
            if (y > 0) r.insert(base + (y - 1) * nx + x);
            if (y + 1 < nx) r.insert(base + (y + 1) * nx + x);
        }
}

struct Lcg {
    uint64_t x;
    uint32_t next() {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(x >> 33);
    }
};

Pattern grid(int nx) {
    std::vector<std::set<int32_t>> rows((size_t)nx * nx);
    add_grid(rows, nx, 0);
    return from_rows(rows);
}

Pattern comps() {
    const int32_t n = 400 + 7 + 225;
    std::vector<std::set<int32_t>> rows(n);
    add_grid(rows, 20, 0);
    add_grid(rows, 15, 407);
    Lcg g{5};
    std::set<int32_t> extra;
    while (extra.size() < 80) extra.insert((int32_t)(g.next() % n));
    rows[3].insert(extra.begin(), extra.end());
    return from_rows(rows);
}

Pattern band() {
    const int32_t n = 500;
    std::vector<std::set<int32_t>> rows(n);
    Lcg g{11};
    for (int k = 0; k < 3000; ++k) {
        const int32_t r = (int32_t)(g.next() % n);
        const int32_t c = r + (int32_t)(g.next() % 35) - 30;
        rows[r].insert(std::max(0, std::min(n - 1, c)));
    }
    return from_rows(rows);
}

uint64_t hash_words(uint64_t h, const int32_t* v, size_t k) {
    for (size_t i = 0; i < k; ++i) h = (h ^ (uint64_t)(uint32_t)v[i]) * 1099511628211ull;
    return h;
}

void set_knobs(int leaf, int threads) {
    setenv("EIGSOL_MF_LEAF", std::to_string(leaf).c_str(), 1);
    setenv("EIGSOL_MF_THREADS", std::to_string(threads).c_str(), 1);
}

constexpr double kFreeBytes = 64.0 * 1073741824.0;

void run_case(const char* name, const Pattern& p, int leaf, int threads) {
    set_knobs(leaf, threads);
    for (int dtype : {EIGSOL_F64, EIGSOL_C128}) {
        MfHost* X = mf_host_new();
        const int rc = mf_prepare(p.n, p.rp, p.ci, dtype, kFreeBytes, X);
        const MfStats& s = mf_host_stats(X);
        uint64_t hp = 14695981039346656037ull, hf = hp;
        if (rc == EIGSOL_OK) {
            hp = hash_words(hp, X->P.perm.data(), X->P.perm.size());
            for (const dev::MfFront& f : X->P.fr) {
                const int32_t q[4] = {f.c0, f.ns, f.ms, f.parent};
                hf = hash_words(hf, q, 4);
            }
        }
        std::printf("case %s %s %d %lld %lld %lld %lld %.17g %.17g %.17g %d %016llx %016llx\n", name,
                    dtype == EIGSOL_F64 ? "f64" : "c128", rc, (long long)s.fronts, (long long)s.heights,
                    (long long)s.max_front, (long long)s.max_pivots, s.factor_entries, s.front_entries, s.flops,
                    rc == EIGSOL_OK ? 1 : 0, (unsigned long long)hp, (unsigned long long)hf);
        mf_host_free(X);
    }
}

void run_cancel(const Pattern& p, int leaf) {
    set_knobs(leaf, 1);
    for (int dtype : {EIGSOL_F64, EIGSOL_C128}) {
        const char* dn = dtype == EIGSOL_F64 ? "f64" : "c128";
        {
            std::atomic<bool> stop{false}, started{false};
            std::thread t([&] {
                while (!started.load(std::memory_order_acquire)) std::this_thread::yield();
                const auto t0 = std::chrono::steady_clock::now();
                while (std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(1)) {}
                stop.store(true);
            });
            MfHost* X = mf_host_new();
            started.store(true, std::memory_order_release);
            const int rc = mf_prepare(p.n, p.rp, p.ci, dtype, kFreeBytes, X, &stop);
            t.join();
            mf_host_free(X);
            std::printf("cancel late %s %d\n", dn, rc);
        }
        {
            std::atomic<bool> stop{true};
            MfHost* X = mf_host_new();
            const int rc = mf_prepare(p.n, p.rp, p.ci, dtype, kFreeBytes, X, &stop);
            mf_host_free(X);
            std::printf("cancel early %s %d\n", dn, rc);
        }
    }
}

}  // namespace

int main() {
    run_case("grid12", grid(12), 500, 1);
    run_case("grid20", grid(20), 4, 1);
    run_case("grid30", grid(30), 16, 1);
    run_case("grid45", grid(45), 24, 1);
    const Pattern g160 = grid(160);
    run_case("grid160_t1", g160, 64, 1);
    run_case("grid160_t3", g160, 64, 3);
    run_case("grid160_t8", g160, 64, 8);
    run_case("comps", comps(), 16, 1);
    run_case("band", band(), 16, 1);
    run_cancel(g160, 64);
    run_case("grid160_after", g160, 64, 8);
    return 0;
}
