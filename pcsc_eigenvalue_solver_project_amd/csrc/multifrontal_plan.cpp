// The host half of the nested-dissection multifrontal LU (the algorithm: multifrontal.hip's header):
// symmetric graph, threaded nested dissection, symbolic structure, and the launch and solve tables
// that multifrontal.hip uploads.  It never touches the device - gmres.hip runs mf_prepare on a
// second host thread with a cancel flag - and it is plain C++: no HIP header, so it also builds
// alone for the host (tests/cpp/mf_plan_host.cpp), under a sanitizer where wanted.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <numeric>
#include <thread>
#include <utility>
#include <vector>

#include "multifrontal_plan.hpp"

namespace eigsol {

namespace {

struct SymGraph {
    std::vector<int64_t> ptr;
    std::vector<int32_t> adj;
};

// fn(begin, end) over [0, n) in contiguous chunks on up to nth host threads
template <class Fn>
void par_for(int64_t n, int nth, Fn fn) {
    if (nth <= 1 || n < 4096) { fn((int64_t)0, n); return; }
    std::vector<std::thread> th;
    const int64_t chunk = (n + nth - 1) / nth;
    try {
        for (int t = 1; t < nth; ++t) {
            const int64_t b = t * chunk, e = std::min(n, b + chunk);
            if (b < e) th.emplace_back(fn, b, e);
        }
    } catch (const std::exception&) {
        for (auto& x : th) x.join();
        fn(chunk, n);   // no more threads: the rest on this one
        fn((int64_t)0, std::min(n, chunk));
        return;
    }
    fn((int64_t)0, std::min(n, chunk));
    for (auto& x : th) x.join();
}

int host_threads() {
    int nth = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (const char* e = std::getenv("EIGSOL_MF_THREADS")) nth = std::max(1, std::atoi(e));
    return nth;
}

// pattern of M + M^T without the diagonal, each list sorted and unique: M's rows merged with the
// rows of its transpose (a counting-sort transpose keeps them sorted)
bool sym_graph(int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, SymGraph& g,
               const std::atomic<bool>* stop = nullptr) {
    const int nth = host_threads();
    auto stopped = [&]() { return stop && stop->load(std::memory_order_relaxed); };
    std::vector<int64_t> tp(n + 1, 0);
    for (int64_t e = 0; e < (int64_t)rp[n]; ++e) ++tp[ci[e] + 1];
    for (int64_t i = 0; i < n; ++i) tp[i + 1] += tp[i];
    if (stopped()) return false;
    std::vector<int32_t> tc(rp[n]);
    {
        std::vector<int64_t> fill(tp.begin(), tp.end() - 1);
        for (int64_t i = 0; i < n; ++i) {
            if ((i & 65535) == 0 && stopped()) return false;
            for (int32_t e = rp[i]; e < rp[i + 1]; ++e) tc[fill[ci[e]]++] = (int32_t)i;
        }
    }
    // merge row i of M and of M^T (both ascending), without i and repeats; count, then fill
    auto merge = [&](int64_t i, int32_t* out) -> int64_t {
        int64_t a = rp[i], ae = rp[i + 1], b = tp[i], be = tp[i + 1], k = 0;
        int32_t last = -1;
        while (a < ae || b < be) {
            int32_t c;
            if (b >= be || (a < ae && ci[a] <= tc[b])) c = ci[a++];
            else c = tc[b++];
            if (c == i || c == last) continue;
            last = c;
            if (out) out[k] = c;
            ++k;
        }
        return k;
    };
    g.ptr.assign(n + 1, 0);
    par_for(n, nth, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) {
            if ((i & 65535) == 0 && stopped()) return;
            g.ptr[i + 1] = merge(i, nullptr);
        }
    });
    if (stopped()) return false;
    for (int64_t i = 0; i < n; ++i) g.ptr[i + 1] += g.ptr[i];
    if (stopped()) return false;
    g.adj.resize(g.ptr[n]);
    par_for(n, nth, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) {
            if ((i & 65535) == 0 && stopped()) return;
            merge(i, g.adj.data() + g.ptr[i]);
        }
    });
    return !stopped();
}

struct NdNode {
    std::vector<int32_t> members;
    int32_t parent;
    std::vector<int32_t> key;   // position in the dissection (independent of thread timing)
};

// Nested dissection of the vertices of g: tree nodes (leaves and separators) with parents, in a
// canonical order (sorted by key: the path of choices from the whole graph to the node's piece).
// Pieces are dissected by a pool of host threads (they touch disjoint vertex sets; a piece's BFS
// reads its neighbours' set tags with relaxed atomics); the tree does not depend on the timing.
bool nested_dissection(int64_t n, const SymGraph& g, int leaf, std::vector<NdNode>& tree,
                       const std::atomic<bool>* stop) {
    struct Task {
        std::vector<int32_t> nodes;
        int32_t parent;
        std::vector<int32_t> key;
    };
    std::vector<Task> stack;
    {
        Task t;
        t.nodes.resize(n);
        std::iota(t.nodes.begin(), t.nodes.end(), 0);
        t.parent = -1;
        stack.push_back(std::move(t));
    }
    // per-vertex state in one record, so a neighbour test touches one cache line: the piece tag
    // (written by the piece's owner, read by the neighbouring pieces' BFS), the BFS stamp and level
    struct Vs {
        int64_t tag, seen;
        int32_t level;
    };
    std::vector<Vs> vs(n, Vs{-1, -1, 0});
    // pseudo-peripheral restarts per piece.  1M convection-diffusion: 2 / 1 / 0
    // rounds -> 1.374e8 / 1.368e8 / 1.47e8 factor entries, 1.13e11 / 1.12e11 / 1.83e11 flops; on the box
    // the set-up is the same for 1 and 2 (0.63-0.67 s) and the solve 1.55 against 1.57 ms: 2 stays
    constexpr int pp_rounds = 2;
    std::atomic<int64_t> stamp{0}, bstamp{0};
    std::mutex mu;
    std::condition_variable cv;
    int active = 0;
    bool aborted = false;
    auto tag_of = [&](int32_t v) { return __atomic_load_n(&vs[v].tag, __ATOMIC_RELAXED); };
    auto add_node = [&](std::vector<int32_t>&& members, int32_t parent, std::vector<int32_t> key) -> int32_t {
        std::lock_guard<std::mutex> lk(mu);
        tree.push_back(NdNode{std::move(members), parent, std::move(key)});
        return (int32_t)tree.size() - 1;
    };
    auto push_task = [&](Task&& t) {
        std::lock_guard<std::mutex> lk(mu);
        stack.push_back(std::move(t));
        cv.notify_one();
    };
    auto work = [&]() {
        std::vector<int32_t> q;
        // raised inside a BFS once *stop is seen (checked every 64K visits: a whole-graph BFS of the
        // top piece takes tens of ms), the task then abandons the dissection
        bool cut = false;
        // BFS inside the piece tagged `tag` from root: q holds the visit order, vs[].level the levels
        auto bfs = [&](int32_t root, int64_t tag) -> int32_t {
            const int64_t b = ++bstamp;
            q.clear();
            q.push_back(root);
            vs[root].seen = b;
            vs[root].level = 0;
            int32_t depth = 0;
            for (size_t h = 0; h < q.size(); ++h) {
                const int32_t v = q[h];
                if ((h & 65535) == 65535 && stop && stop->load(std::memory_order_relaxed)) {
                    cut = true;
                    return depth;
                }
                const int32_t lw = vs[v].level + 1;
                for (int64_t e = g.ptr[v]; e < g.ptr[v + 1]; ++e) {
                    const int32_t w = g.adj[e];
                    if (tag_of(w) != tag || vs[w].seen == b) continue;
                    vs[w].seen = b;
                    vs[w].level = lw;
                    depth = std::max(depth, lw);
                    q.push_back(w);
                }
            }
            return depth;
        };
        auto sub_degree = [&](int32_t v, int64_t tag) {
            int32_t dgr = 0;
            for (int64_t e = g.ptr[v]; e < g.ptr[v + 1]; ++e) dgr += tag_of(g.adj[e]) == tag;
            return dgr;
        };
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return aborted || !stack.empty() || active == 0; });
                if (aborted || stack.empty()) { cv.notify_all(); return; }
                t = std::move(stack.back());
                stack.pop_back();
                ++active;
            }
            auto done = [&]() {
                std::lock_guard<std::mutex> lk(mu);
                --active;
                if (active == 0 && stack.empty()) cv.notify_all();
            };
            auto abort_task = [&]() {
                std::lock_guard<std::mutex> lk(mu);
                aborted = true;
                --active;
                cv.notify_all();
            };
            if (cut || (stop && stop->load(std::memory_order_relaxed))) {
                abort_task();
                return;
            }
            const int64_t sz = (int64_t)t.nodes.size();
            if (sz == 0) { done(); continue; }
            if (sz <= leaf) {
                add_node(std::move(t.nodes), t.parent, std::move(t.key));
                done();
                continue;
            }
            const int64_t tag = ++stamp;
            for (int32_t v : t.nodes) __atomic_store_n(&vs[v].tag, tag, __ATOMIC_RELAXED);
            // from the piece's first vertex: connectivity, and the first pseudo-peripheral level set
            const int32_t depth0 = bfs(t.nodes[0], tag);
            if (cut) {
                abort_task();
                return;
            }
            if ((int64_t)q.size() < sz) {
                // disconnected: components (in the order of their first vertex in the piece); the
                // small ones packed into leaves, the others new pieces
                std::vector<std::vector<int32_t>> comps;
                const int64_t b0 = vs[t.nodes[0]].seen;   // this piece's first BFS; later ones are larger
                comps.push_back(q);
                for (int32_t v : t.nodes) {
                    if (vs[v].seen >= b0) continue;
                    bfs(v, tag);
                    if (cut) break;
                    comps.push_back(q);
                }
                if (cut) {
                    abort_task();
                    return;
                }
                std::vector<int32_t> pack;
                int32_t slot = 0;
                auto key_at = [&](int32_t k) {
                    std::vector<int32_t> kk = t.key;
                    kk.push_back(k);
                    return kk;
                };
                for (auto& c : comps) {
                    if ((int64_t)c.size() > leaf) {
                        push_task(Task{std::move(c), t.parent, key_at(slot++)});
                        continue;
                    }
                    if ((int64_t)(pack.size() + c.size()) > leaf) {
                        add_node(std::move(pack), t.parent, key_at(slot++));
                        pack.clear();
                    }
                    pack.insert(pack.end(), c.begin(), c.end());
                }
                if (!pack.empty()) add_node(std::move(pack), t.parent, key_at(slot++));
                done();
                continue;
            }
            // pseudo-peripheral root (George-Liu): restart from a minimum-degree vertex of the last
            // level while the eccentricity grows
            int32_t root = t.nodes[0];
            int32_t ecc = depth0;   // q and the levels are still those of the BFS from root
            for (int round = 0; round < pp_rounds; ++round) {
                int32_t best = -1, bd = INT32_MAX;
                for (size_t h = q.size(); h-- > 0;) {
                    const int32_t v = q[h];
                    if (vs[v].level != ecc) break;
                    const int32_t dv = sub_degree(v, tag);
                    if (dv < bd || (dv == bd && v < best)) { bd = dv; best = v; }
                }
                const int32_t e2 = bfs(best, tag);
                if (e2 <= ecc) {
                    if (e2 < ecc) ecc = bfs(root, tag);   // restore the levels of the better root
                    break;
                }
                root = best;
                ecc = e2;
            }
            if (cut) {
                abort_task();
                return;
            }
            const int32_t nlev = ecc + 1;
            if (nlev < 3) {   // no level structure to cut: one dense front
                add_node(std::move(t.nodes), t.parent, std::move(t.key));
                done();
                continue;
            }
            std::vector<int64_t> cnt(nlev, 0);
            for (int32_t v : t.nodes) ++cnt[vs[v].level];
            int32_t m = 1;
            {
                int64_t cum = 0;
                for (int32_t l = 0; l < nlev; ++l) {
                    if (2 * (cum + cnt[l] / 2) >= sz) { m = l; break; }
                    cum += cnt[l];
                }
                m = std::max(1, std::min(nlev - 2, m));
            }
            // separator: the vertices of level m that touch level m + 1; the rest of level m joins A
            std::vector<int32_t> A, B, Sep;
            for (int32_t v : t.nodes) {
                const int32_t l = vs[v].level;
                if (l < m) A.push_back(v);
                else if (l > m) B.push_back(v);
                else {
                    bool touch = false;
                    for (int64_t e = g.ptr[v]; e < g.ptr[v + 1] && !touch; ++e)
                        touch = tag_of(g.adj[e]) == tag && vs[g.adj[e]].level == m + 1;
                    (touch ? Sep : A).push_back(v);
                }
            }
            std::vector<int32_t>().swap(t.nodes);
            std::vector<int32_t> ka = t.key, kb = t.key;
            ka.push_back(0);
            kb.push_back(1);
            const int32_t id = add_node(std::move(Sep), t.parent, std::move(t.key));
            push_task(Task{std::move(A), id, std::move(ka)});
            push_task(Task{std::move(B), id, std::move(kb)});
            done();
        }
    };
    int nth = host_threads();
    if (n < 20000) nth = 1;
    std::vector<std::thread> pool;
    try {
        for (int i = 1; i < nth; ++i) pool.emplace_back(work);
    } catch (const std::exception&) {   // fewer threads: the others do the work
    }
    work();
    for (auto& th : pool) th.join();
    if (aborted) return false;
    // canonical order: by key; parents renumbered
    std::vector<int32_t> ord(tree.size());
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return tree[x].key < tree[y].key; });
    std::vector<int32_t> newid(tree.size());
    for (size_t i = 0; i < ord.size(); ++i) newid[ord[i]] = (int32_t)i;
    std::vector<NdNode> sorted;
    sorted.reserve(tree.size());
    for (int32_t o : ord) {
        NdNode nd = std::move(tree[o]);
        if (nd.parent >= 0) nd.parent = newid[nd.parent];
        std::vector<int32_t>().swap(nd.key);
        sorted.push_back(std::move(nd));
    }
    tree.swap(sorted);
    return true;
}

}  // namespace

bool mf_plan(int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int leaf, bool cplx_flops,
             MfPlan& P, double max_front_entries, const std::atomic<bool>* stop) {
    static const bool dbg = std::getenv("EIGSOL_MF_DEBUG") != nullptr;
    auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[mf] %s %.3f s\n", what, std::chrono::duration<double>(t - tp).count());
        tp = t;
    };
    // the graph relabelled in breadth-first order (neighbours get nearby labels: the many BFS
    // passes of the dissection then walk memory locally whatever the caller's numbering)
    SymGraph g;
    std::vector<int32_t> ord(n);   // label -> caller's index
    auto stopped = [&]() { return stop && stop->load(std::memory_order_relaxed); };
    {
        SymGraph g0;
        if (!sym_graph(n, rp, ci, g0, stop)) return false;
        lap("graph: symmetric pattern");
        std::vector<char> done(n, 0);
        int64_t head = 0, tail = 0;
        for (int64_t s0 = 0; s0 < n; ++s0) {
            if (done[s0]) continue;
            done[s0] = 1;
            ord[tail++] = (int32_t)s0;
            while (head < tail) {
                if ((head & 65535) == 0 && stopped()) return false;
                const int32_t v = ord[head++];
                for (int64_t e = g0.ptr[v]; e < g0.ptr[v + 1]; ++e)
                    if (!done[g0.adj[e]]) { done[g0.adj[e]] = 1; ord[tail++] = g0.adj[e]; }
            }
        }
        if (stopped()) return false;
        lap("graph: breadth-first labels");
        std::vector<int32_t> lab(n);
        for (int64_t k = 0; k < n; ++k) lab[ord[k]] = (int32_t)k;
        g.ptr.assign(n + 1, 0);
        for (int64_t k = 0; k < n; ++k) g.ptr[k + 1] = g.ptr[k] + (g0.ptr[ord[k] + 1] - g0.ptr[ord[k]]);
        g.adj.resize(g0.adj.size());
        par_for(n, host_threads(), [&](int64_t b, int64_t e) {
            for (int64_t k = b; k < e; ++k) {
                const int32_t v = ord[k];
                int64_t o = g.ptr[k];
                for (int64_t x = g0.ptr[v]; x < g0.ptr[v + 1]; ++x) g.adj[o++] = lab[g0.adj[x]];
                std::sort(g.adj.begin() + g.ptr[k], g.adj.begin() + o);
            }
        });
    }
    lap("graph");
    std::vector<NdNode> tree;
    if (!nested_dissection(n, g, leaf, tree, stop)) return false;
    lap("dissection");
    // postorder numbering: children before parents, each tree node one contiguous column range
    const int64_t nt = (int64_t)tree.size();
    P.nt = nt;
    std::vector<int32_t> post;   // tree node of each front (postorder)
    post.reserve(nt);
    {
        std::vector<std::vector<int32_t>> kids(nt);
        std::vector<int32_t> roots;
        for (int64_t i = 0; i < nt; ++i) {
            if (tree[i].parent < 0) roots.push_back((int32_t)i);
            else kids[tree[i].parent].push_back((int32_t)i);
        }
        std::vector<std::pair<int32_t, size_t>> st;
        for (int32_t r : roots) {
            st.push_back({r, 0});
            while (!st.empty()) {
                auto& top = st.back();
                if (top.second < kids[top.first].size()) {
                    const int32_t c = kids[top.first][top.second++];
                    st.push_back({c, 0});
                } else {
                    post.push_back(top.first);
                    st.pop_back();
                }
            }
        }
    }
    std::vector<int32_t> front_of_node(nt);
    for (int64_t s = 0; s < nt; ++s) front_of_node[post[s]] = (int32_t)s;
    P.perm.assign(n, 0);
    P.iperm.assign(n, 0);
    P.snode.assign(n, 0);
    P.fr.assign(nt, dev::MfFront{});
    auto& fr = P.fr;
    {
        int32_t c = 0;
        for (int64_t s = 0; s < nt; ++s) {
            const NdNode& nd = tree[post[s]];
            fr[s].c0 = c;
            fr[s].ns = (int32_t)nd.members.size();
            fr[s].parent = nd.parent < 0 ? -1 : front_of_node[nd.parent];
            for (int32_t v : nd.members) {
                P.perm[c] = v;
                P.iperm[v] = c;
                P.snode[c] = (int32_t)s;
                ++c;
            }
        }
    }
    std::vector<NdNode>().swap(tree);
    // children lists (postorder, i.e. the fixed extend-add order)
    auto& chl = P.chl;
    {
        std::vector<std::vector<int32_t>> ch(nt);
        for (int64_t s = 0; s < nt; ++s)
            if (fr[s].parent >= 0) ch[fr[s].parent].push_back((int32_t)s);
        for (int64_t s = 0; s < nt; ++s) {
            fr[s].ch0 = (int32_t)chl.size();
            chl.insert(chl.end(), ch[s].begin(), ch[s].end());
            fr[s].ch1 = (int32_t)chl.size();
        }
    }
    // heights (a leaf 0, a parent one above its highest child) and the per-height front lists
    // (descending ns: each panel's fronts are a prefix)
    P.height.assign(nt, 0);
    P.H = 0;
    for (int64_t s = 0; s < nt; ++s) {
        for (int32_t k = fr[s].ch0; k < fr[s].ch1; ++k) P.height[s] = std::max(P.height[s], P.height[chl[k]] + 1);
        P.H = std::max(P.H, P.height[s]);
    }
    P.hstart.assign(P.H + 2, 0);
    {
        std::vector<std::vector<int32_t>> byh(P.H + 1);
        for (int64_t s = 0; s < nt; ++s) byh[P.height[s]].push_back((int32_t)s);
        for (int32_t h = 0; h <= P.H; ++h) {
            std::stable_sort(byh[h].begin(), byh[h].end(), [&](int32_t a, int32_t b) { return fr[a].ns > fr[b].ns; });
            P.lists.insert(P.lists.end(), byh[h].begin(), byh[h].end());
            P.hstart[h + 1] = (int64_t)P.lists.size();
        }
    }
    // symbolic: struct(s) = indices >= c1 reached from s's rows in M + M^T or through a child's
    // struct (each list ascending).  A front needs only its children's lists, so the fronts of one
    // height are independent: they run on the host threads (a mark array per thread), height after
    // height, and the lists are concatenated in front order -- the same arrays as a serial pass.
    auto& sidx = P.sidx;
    auto& sof = P.sof;
    sof.assign(nt + 1, 0);
    {
        std::vector<std::vector<int32_t>> lists(nt);
        std::atomic<bool> over{false};
        std::atomic<double> fe_run{0.0};
        const int nth = host_threads();
        std::vector<std::vector<int32_t>> marks(std::max(1, nth));
        auto one = [&](int32_t s, std::vector<int32_t>& mark) {
            const int32_t c0 = fr[s].c0, c1 = c0 + fr[s].ns;
            std::vector<int32_t>& lst = lists[s];
            for (int32_t i = c0; i < c1; ++i) {
                const int32_t v = P.perm[i];
                for (int64_t e = g.ptr[v]; e < g.ptr[v + 1]; ++e) {
                    const int32_t j = P.iperm[g.adj[e]];
                    if (j >= c1 && mark[j] != s) { mark[j] = s; lst.push_back(j); }
                }
            }
            for (int32_t k = fr[s].ch0; k < fr[s].ch1; ++k)
                for (int32_t j : lists[chl[k]])
                    if (j >= c1 && mark[j] != s) { mark[j] = s; lst.push_back(j); }
            std::sort(lst.begin(), lst.end());
            const double d = (double)fr[s].ns + (double)lst.size();
            double cur = fe_run.load(std::memory_order_relaxed);
            while (!fe_run.compare_exchange_weak(cur, cur + d * d, std::memory_order_relaxed)) {}
            if (cur + d * d > max_front_entries) over.store(true, std::memory_order_relaxed);
        };
        for (int32_t h = 0; h <= P.H; ++h) {
            const int64_t b = P.hstart[h], m = P.hstart[h + 1] - b;
            const int use = m < 8 ? 1 : (int)std::min<int64_t>(std::max(1, nth), m);
            auto run = [&](int t) {
                std::vector<int32_t>& mark = marks[t];
                if (mark.empty()) mark.assign(n, -1);
                for (int64_t k = t; k < m; k += use) {   // fronts dealt round-robin: sizes vary by position
                    if (over.load(std::memory_order_relaxed) || stopped()) return;
                    one(P.lists[b + k], mark);
                }
            };
            if (use <= 1) {
                run(0);
            } else {
                std::vector<std::thread> th;
                try {
                    for (int t = 1; t < use; ++t) th.emplace_back(run, t);
                } catch (const std::exception&) {
                    for (auto& x : th) x.join();
                    th.clear();
                    for (int t = 1; t < use; ++t) run(t);   // no more threads: this one does the rest
                }
                run(0);
                for (auto& x : th) x.join();
            }
            if (over.load() || stopped()) return false;
        }
        int64_t tot = 0;
        for (int64_t s = 0; s < nt; ++s) tot += (int64_t)lists[s].size();
        sidx.reserve(tot);
        for (int64_t s = 0; s < nt; ++s) {
            sidx.insert(sidx.end(), lists[s].begin(), lists[s].end());
            std::vector<int32_t>().swap(lists[s]);
            sof[s + 1] = (int64_t)sidx.size();
            fr[s].ms = (int32_t)(sof[s + 1] - sof[s]);
            fr[s].sof = sof[s];
            fr[s].d = fr[s].ns + fr[s].ms;
        }
    }
    std::vector<int64_t>().swap(g.ptr);
    std::vector<int32_t>().swap(g.adj);
    // labels -> the caller's indices
    for (int64_t c = 0; c < n; ++c) {
        P.perm[c] = ord[P.perm[c]];
        P.iperm[P.perm[c]] = (int32_t)c;
    }
    lap("symbolic");
    // sizes and work
    for (int64_t s = 0; s < nt; ++s) {
        const double d = fr[s].d, ns = fr[s].ns;
        fr[s].off = (int64_t)P.fe;
        fr[s].uoff = P.uo;
        P.uo += fr[s].ms;
        P.fe += d * d;
        P.fac += ns * (2.0 * d - ns);
        // sum_{k < ns} 2 (d - k - 1)^2 multiply-adds ~ 2 (ns d^2 - ns^2 d + ns^3 / 3)
        P.flops += 2.0 * (ns * d * d - ns * ns * d + ns * ns * ns / 3.0);
        P.maxd = std::max<int64_t>(P.maxd, fr[s].d);
        P.maxns = std::max<int64_t>(P.maxns, fr[s].ns);
    }
    if (cplx_flops) P.flops *= 4.0;
    lap("sizes");
    // parent positions of every child's struct entries
    P.cmap.assign(sidx.size(), 0);
    for (int64_t s = 0; s < nt; ++s) {
        const int32_t p = fr[s].parent;
        if (p < 0) {
            if (fr[s].ms) return false;   // a root reaches nothing past itself
            continue;
        }
        const int32_t pc0 = fr[p].c0, pc1 = pc0 + fr[p].ns;
        const int32_t* ps = sidx.data() + sof[p];
        const int32_t pm = fr[p].ms;
        int32_t cur = 0;
        for (int64_t e = sof[s]; e < sof[s + 1]; ++e) {
            const int32_t j = sidx[e];
            if (j < pc0) return false;   // struct(s) must lie in the ancestors
            if (j < pc1) P.cmap[e] = j - pc0;
            else {
                while (cur < pm && ps[cur] < j) ++cur;   // both ascending
                if (cur == pm || ps[cur] != j) return false;
                P.cmap[e] = fr[p].ns + cur;
            }
        }
    }
    lap("parent maps");
    return true;
}

// The host half of the factor: plan, bounds, entry destinations, launch and solve tables.  Needs
// no device (free_bytes: the device memory the fronts may take), so gmres.hip runs it on a second
// host thread beside the natural-order fill attempt.
static int mf_prepare_host(int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, bool cplx_s,
                           double free_bytes, MfHost& X, const std::atomic<bool>* stop) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const int NB = cplx_s ? kMfPanelC128 : kMfPanelF64;
    const int64_t sb = cplx_s ? 16 : 8;
    X.n = n;
    X.nb = NB;
    X.sb = sb;
    int leaf = 64;
    if (const char* e = std::getenv("EIGSOL_MF_LEAF")) leaf = std::max(4, std::atoi(e));
    MfPlan& P = X.P;
    double cap = 0.45 * free_bytes;
    if (const char* e = std::getenv("EIGSOL_MF_MAX_GB")) cap = std::min(cap, std::atof(e) * 1073741824.0);
    if (!mf_plan(n, rp, ci, leaf, cplx_s, P, cap / (double)sb, stop)) return EIGSOL_E_UNSUPPORTED;
    const int64_t nt = P.nt;
    auto& fr = P.fr;
    const auto& chl = P.chl;
    const auto& sidx = P.sidx;
    const auto& sof = P.sof;
    const auto& lists = P.lists;
    const auto& hstart = P.hstart;
    const int32_t H = P.H;
    const double fe = P.fe, fac = P.fac;
    MfStats& stt = X.stt;
    stt.fronts = nt;
    stt.heights = H + 1;
    stt.max_front = P.maxd;
    stt.max_pivots = P.maxns;
    stt.front_entries = fe;
    stt.factor_entries = fac;
    stt.flops = P.flops;
    // bounds: device memory for the fronts, the solve kernels' LDS, the work
    const double lds_max = 120.0 * 1024.0;
    if (fe * (double)sb > cap || (double)(P.maxns + P.maxd) * (double)sb > lds_max || P.flops > 4e13)
        return EIGSOL_E_UNSUPPORTED;
    // destinations of M's entries (the caller's numbering) in the fronts
    const int64_t nnz = rp[n];
    X.nnz = nnz;
    auto& dst = X.dst;
    dst.assign(nnz, 0);
    auto pos_in = [&](int32_t s, int32_t j) -> int64_t {
        const int32_t c0 = fr[s].c0;
        if (j < c0 + fr[s].ns) return j - c0;
        const int32_t* b = sidx.data() + sof[s];
        const int64_t k = std::lower_bound(b, b + fr[s].ms, j) - b;
        return (k < fr[s].ms && b[k] == j) ? fr[s].ns + k : -1;
    };
    std::atomic<bool> bad{false};
    par_for(n, host_threads(), [&](int64_t rb, int64_t re) {
        for (int64_t r = rb; r < re; ++r)
            for (int32_t e = rp[r]; e < rp[r + 1]; ++e) {
                const int32_t i = P.iperm[r], j = P.iperm[ci[e]];
                const int32_t s = P.snode[std::min(i, j)];
                const int64_t pi = pos_in(s, i), pj = pos_in(s, j);
                if (pi < 0 || pj < 0) { bad.store(true); return; }   // not in the front: an inconsistent plan
                dst[e] = fr[s].off + pi + pj * (int64_t)fr[s].d;
            }
    });
    if (bad.load()) return EIGSOL_E_UNSUPPORTED;
    // launch tables: extend-add (child, first column) per (height, child rank); trailing-update
    // tiles (front, tile row, tile column) per (height, panel)
    using Launch = MfLaunch;
    auto& plan = X.plan;
    auto& tab = X.tab;
    for (int32_t h = 0; h <= H; ++h) {
        const int32_t* L = lists.data() + hstart[h];
        const int64_t cnt = hstart[h + 1] - hstart[h];
        int32_t maxch = 0, maxq = 0;
        for (int64_t t = 0; t < cnt; ++t) {
            maxch = std::max(maxch, fr[L[t]].ch1 - fr[L[t]].ch0);
            maxq = std::max(maxq, (fr[L[t]].ns + NB - 1) / NB);
        }
        for (int32_t j = 0; j < maxch; ++j) {
            const int64_t o = (int64_t)tab.size();
            for (int64_t t = 0; t < cnt; ++t) {
                const dev::MfFront& p = fr[L[t]];
                if (p.ch1 - p.ch0 <= j) continue;
                const int32_t c = chl[p.ch0 + j];
                for (int32_t c0 = 0; c0 < fr[c].ms; c0 += 64) { tab.push_back(c); tab.push_back(c0); }
            }
            const int64_t k = ((int64_t)tab.size() - o) / 2;
            if (k) plan.push_back(Launch{0, h, j, o, k});
        }
        for (int32_t q = 0; q < maxq; ++q) {
            int64_t np = 0;
            while (np < cnt && fr[L[np]].ns > q * NB) ++np;
            plan.push_back(Launch{1, h, q, hstart[h], np});
            const int64_t o = (int64_t)tab.size();
            for (int64_t t = 0; t < np; ++t) {
                const dev::MfFront& f = fr[L[t]];
                const int32_t c1 = std::min(f.ns, (q + 1) * NB), m = f.d - c1;
                const int32_t nt64 = (m + 63) / 64;
                for (int32_t a = 0; a < nt64; ++a)
                    for (int32_t b = 0; b < nt64; ++b) { tab.push_back(L[t]); tab.push_back(a); tab.push_back(b); }
            }
            const int64_t k = ((int64_t)tab.size() - o) / 3;
            if (k) plan.push_back(Launch{2, h, q, o, k});
        }
    }
    // solve plan: fronts with many pivots or rows are solved by one workgroup per 64-row block
    // (mf_big_*), the others by one workgroup each (mf_fwd / mf_bwd)
    int big_ns = 96;
    constexpr int big_d = 256;
    if (const char* e = std::getenv("EIGSOL_MF_BIG_NS")) big_ns = std::atoi(e);
    auto &slists = X.slists, &tabf = X.tabf, &tabb = X.tabb;
    MfSolveTables& T = X.T;
    T.sstart.assign(H + 2, 0);
    for (auto* v : {&T.nsmall, &T.nbig, &T.foff, &T.fcnt, &T.boff, &T.bcnt}) v->assign(H + 1, 0);
    for (auto* v : {&T.lds_fwd, &T.lds_bwd, &T.lds_bbig, &T.lds_asm, &T.lds_asm2}) v->assign(H + 1, 0);
    bool inv_on = true;
    constexpr int inv_d = 256;   // 256 / 384 / 512: 1.71 / 1.72 / 1.72 ms per 1M iteration (tools/mf_grid.sh)
    if (const char* e = std::getenv("EIGSOL_MF_INVFORM")) inv_on = std::atoi(e) != 0;
    int32_t& nflag = X.nflag;
    int64_t& zsz = X.zsz;
    for (int32_t h = 0; h <= H; ++h) {
        std::vector<int32_t> big;
        for (int64_t t = hstart[h]; t < hstart[h + 1]; ++t) {
            dev::MfFront& q = fr[lists[t]];
            q.flag0 = -1;
            q.zoff = 0;
            // fronts of at most 64 pivots and inv_d rows stay one-workgroup fronts (inverse form)
            const bool inv_ok = inv_on && q.ns <= 64 && q.d <= inv_d;
            const bool is_big = big_ns > 0 && (q.ns >= big_ns || (q.d >= big_d && !inv_ok));
            if (is_big) big.push_back(lists[t]);
            else slists.push_back(lists[t]);
        }
        T.nsmall[h] = (int64_t)slists.size() - T.sstart[h];
        T.nbig[h] = (int64_t)big.size();
        slists.insert(slists.end(), big.begin(), big.end());
        T.sstart[h + 1] = (int64_t)slists.size();
        T.foff[h] = (int64_t)tabf.size() / 2;
        T.boff[h] = (int64_t)tabb.size() / 2;
        for (int32_t b : big) {
            dev::MfFront& q = fr[b];
            const int32_t nblk = (q.ns + 63) / 64, nsb = (q.ms + 63) / 64;
            q.flag0 = nflag;
            q.zoff = zsz;
            nflag += nblk;
            zsz += q.d;
            for (int32_t k = 0; k < nblk + nsb; ++k) { tabf.push_back(b); tabf.push_back(k); }
            for (int32_t k = nblk - 1; k >= 0; --k) { tabb.push_back(b); tabb.push_back(k); }
            T.lds_asm[h] = std::max<int32_t>(T.lds_asm[h], (int32_t)(q.ns * sb));
            T.lds_asm2[h] = std::max<int32_t>(T.lds_asm2[h], (int32_t)((q.ns + q.ms) * sb));   // d: mf_big_asm_front2
            T.lds_bbig[h] = std::max<int32_t>(T.lds_bbig[h], (int32_t)(q.ms * sb));
        }
        T.fcnt[h] = (int64_t)tabf.size() / 2 - T.foff[h];
        T.bcnt[h] = (int64_t)tabb.size() / 2 - T.boff[h];
    }
    // inverse forms of the one-workgroup fronts with at most 64 pivots and inv_d rows
    // (mf_invform2_kernel), kept only while the fronts and the forms fit 0.6 of the device memory
    X.inv_list.clear();
    X.gsz = 0;
    for (int64_t s2 = 0; s2 < nt; ++s2) {
        dev::MfFront& q = fr[s2];
        q.goff = -1;
        if (inv_on && q.flag0 < 0 && q.ns <= 64 && q.d <= inv_d) {
            q.goff = (int64_t)fe + X.gsz;
            X.gsz += 2 * (int64_t)q.d * q.ns;
            X.inv_list.push_back((int32_t)s2);
        }
    }
    if (((double)fe + (double)X.gsz) * (double)sb > 0.6 * free_bytes) {
        for (int32_t s2 : X.inv_list) fr[s2].goff = -1;
        X.inv_list.clear();
        X.gsz = 0;
    }
    // the one-workgroup fronts' vectors; the inverse-form branch keeps 256 partial sums after them
    const int32_t inv_lds = X.gsz ? (int32_t)(256 * sb) : 0;
    for (int32_t h = 0; h <= H; ++h)
        for (int64_t t = T.sstart[h]; t < T.sstart[h] + T.nsmall[h]; ++t) {
            const dev::MfFront& q = fr[slists[t]];
            T.lds_fwd[h] = std::max<int32_t>(T.lds_fwd[h], (int32_t)((2 * q.ns + q.ms) * sb) + inv_lds);
            T.lds_bwd[h] = std::max<int32_t>(T.lds_bwd[h], (int32_t)((q.ns + q.ms) * sb) + inv_lds);
        }
    stt.order_seconds = std::chrono::duration<double>(clk::now() - t0).count();
    if (std::getenv("EIGSOL_MF_DEBUG"))
        std::fprintf(stderr, "[mf] plan + maps + tables %.3f s; fronts %lld, heights %d, factor entries %.3g, flops %.3g\n",
                     stt.order_seconds, (long long)nt, H + 1, fac, P.flops);
    return EIGSOL_OK;
}

MfHost* mf_host_new() { return new MfHost(); }
const MfStats& mf_host_stats(const MfHost* X) { return X->stt; }
void mf_host_free(MfHost* X) { delete X; }

int mf_prepare(int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int dtype, double free_bytes,
               MfHost* X, const std::atomic<bool>* stop) {
    if (dtype != EIGSOL_C128 && dtype != EIGSOL_F64) return EIGSOL_E_UNSUPPORTED;
    try {
        return mf_prepare_host(n, rp, ci, dtype == EIGSOL_C128, free_bytes, *X, stop);
    } catch (const std::exception&) {   // host allocation of the plan: decline
        return EIGSOL_E_UNSUPPORTED;
    }
}

}  // namespace eigsol
