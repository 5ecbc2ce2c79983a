// The union-find of mdir_amd/csrc/mdx_unionfind.h under a host memory policy (the __atomic builtins on int32), hammered from 8
// threads and compared with a sequential union-find: the roots must be the component minima, the successful hooks must number
// n minus the components, and the forest invariant parent[x] <= x must hold.  Built and run by tests/test_unionfind_host.py under
// AddressSanitizer + UBSan and, where it links, ThreadSanitizer.  Exit status 0: every edge set agreed.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../mdir_amd/csrc/mdx_unionfind.h"

namespace {

struct HostMem {
    static int32_t load(int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static int32_t cas(int32_t *p, int32_t expected, int32_t desired)
    {
        (void)__atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expected;
    }
    static void store_min(int32_t *p, int32_t v)
    {
        int32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
        }
    }
};

typedef std::vector<std::pair<int32_t, int32_t>> Edges;
constexpr int THREADS = 8;

std::vector<int32_t> sequential(int32_t n, const Edges &edges)
{
    std::vector<int32_t> p(n);
    std::iota(p.begin(), p.end(), 0);
    auto find = [&](int32_t x) {
        while (p[x] != x) x = p[x] = p[p[x]];
        return x;
    };
    for (const auto &e : edges) {
        const int32_t a = find(e.first), b = find(e.second);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
    std::vector<int32_t> root(n);
    for (int32_t i = 0; i < n; ++i) root[i] = find(i);
    return root;
}

int run(const char *name, int32_t n, const Edges &edges)
{
    std::vector<int32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0);
    std::atomic<int64_t> hooks{0};
    std::atomic<int> flags{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
        pool.emplace_back([&, t]() {
            int f = 0;
            int64_t h = 0;
            for (size_t e = t; e < edges.size(); e += THREADS)               // interleaved: neighbours in the list run side by side
                h += mdx::uf_unite<HostMem>(parent.data(), edges[e].first, edges[e].second, (int64_t)n + 1, f);
            hooks += h;
            flags |= f;
        });
    for (auto &th : pool) th.join();
    const std::vector<int32_t> want = sequential(n, edges);
    int64_t components = 0;
    int bad = 0;
    for (int32_t i = 0; i < n; ++i) {
        components += want[i] == i;
        if (parent[i] > i || parent[i] < 0) ++bad;
        if (!bad && mdx::uf_root<HostMem>(parent.data(), i, (int64_t)n + 1) != want[i]) ++bad;
    }
    if (flags.load()) ++bad;
    if (hooks.load() != n - components) ++bad;
    std::printf("%-10s n=%d edges=%zu components=%lld hooks=%lld flags=%d %s\n", name, n, edges.size(), (long long)components,
                (long long)hooks.load(), flags.load(), bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

}  // namespace

int main()
{
    int failed = 0;
    std::mt19937 rng(12345);
    const int32_t n = 20000;

    Edges path;
    for (int32_t i = 0; i + 1 < n; ++i) path.push_back({i, i + 1});
    failed += run("path", n, path);

    Edges star;                                                              // the hub has the LARGEST id: every hook moves the one tree
    for (int32_t i = 0; i + 1 < n; ++i) star.push_back({n - 1, i});
    failed += run("star", n, star);

    Edges permuted = path;                                                   // the path under a permutation of ids and of the edge order
    std::vector<int32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    for (auto &e : permuted) e = {perm[e.first], perm[e.second]};
    std::shuffle(permuted.begin(), permuted.end(), rng);
    failed += run("permuted", n, permuted);

    for (int round = 0; round < 4; ++round) {                                // sparse to dense; duplicates and self-loops included
        Edges random;
        const size_t count = (size_t)n / 4 << round;
        std::uniform_int_distribution<int32_t> pick(0, n - 1);
        for (size_t e = 0; e < count; ++e) random.push_back({pick(rng), pick(rng)});
        failed += run("random", n, random);
    }

    Edges clique;                                                            // every thread contends for one root
    for (int32_t i = 0; i < 300; ++i)
        for (int32_t j = i + 1; j < 300; ++j) clique.push_back({j, i});
    failed += run("clique", 300, clique);

    // the give-up path, without any contention: a forest that init did not write is left alone and flagged
    {
        std::vector<int32_t> broken = {0, 5, 1, 3, 9, 2};
        int f = 0;
        const int made = mdx::uf_unite<HostMem>(broken.data(), 1, 3, 7, f);
        const bool ok = made == 0 && (f & mdx::MDX_UF_GAVE_UP) && broken == std::vector<int32_t>({0, 5, 1, 3, 9, 2});
        std::printf("%-10s %s\n", "give-up", ok ? "ok" : "FAILED");
        failed += !ok;
    }
    return failed ? 1 : 0;
}
