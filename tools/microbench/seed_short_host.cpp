// seed_short_host.cpp — the host sweep of the short seeded division's certificate (platymatch_amd/csrc/pm_seed_short.h:
// div_seeded_short, seed_short_pair_ok).  The device certifies per launch (pm_chi2.hip: seed_cert_kernel); this program evaluates
// the SAME predicate with std::fma and IEEE division over the whole domain — every (ca, cb) with ca + cb < 8 836 = 94^2 — for a
// list of totals, R[s] = fl(T/s), R[0] = 1.
//     seed_short_host            the plain sweep: one line per total, failures expected 0
//     seed_short_host K          the same with every R[s] degraded to fl(R[s] (1 + 2^-K)): shows that the predicate can say no
// Build: c++ -std=c++17 -O2 -ffp-contract=off seed_short_host.cpp -o seed_short_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../platymatch_amd/csrc/pm_seed_short.h"

constexpr int NSEED = 94 * 94;

int main(int argc, char **argv) {
    const int totals[5] = {999, 4096, 19999, 49999, 199999};
    const int k = argc > 1 ? atoi(argv[1]) : 0;
    const double factor = k > 0 ? 1.0 + std::ldexp(1.0, -k) : 1.0;
    const int nthreads = 4;
    for (int it = 0; it < 5; ++it) {
        const double T = (double)totals[it];
        std::vector<double> R(NSEED);
        R[0] = 1.0 * factor;
        for (int s = 1; s < NSEED; ++s) R[s] = (T / (double)s) * factor;
        std::vector<unsigned long long> bad(nthreads, 0), pairs(nthreads, 0);
        std::vector<std::thread> pool;
        for (int w = 0; w < nthreads; ++w)
            pool.emplace_back([&, w]() {
                unsigned long long b = 0, p = 0;
                for (int ca = w; ca < NSEED; ca += nthreads)
                    for (int cb = 0; ca + cb < NSEED; ++cb) {
                        ++p;
                        b += !pm::seed_short_pair_ok(ca, cb, T, R.data(), 0, [](double n, double d) { return n / d; });
                    }
                bad[w] = b, pairs[w] = p;
            });
        for (auto &t : pool) t.join();
        unsigned long long b = 0, p = 0;
        for (int w = 0; w < nthreads; ++w) b += bad[w], p += pairs[w];
        printf("T %d degrade %d pairs %llu short_bad %llu\n", totals[it], k, p, b);
    }
    return 0;
}
