// rcp_window_check.hip -- PROOF by enumeration that the two-instruction window test of rcp_exact (cl2::rcp_window,
// csrc/vecmath.hpp: shift the sign out, add -(1 << 24), one unsigned compare) accepts exactly the bit patterns whose exponent
// field lies in [1, 252], i.e. those the former three-instruction form `((bits >> 23) & 0xFF) - 1 < 252` accepted.  All 2^32
// patterns, on the host: no GPU is needed or used.
//   build: hipcc --offload-arch=gfx950 --cuda-host-only -O3 -std=c++17 -pthread tools/rcp_window_check.hip -o tools/rcp_window_check
//   usage: rcp_window_check        exit status 0 and "0 of 4294967296 patterns differ" when the predicates agree
#include "../clive2_amd/csrc/vecmath.hpp"
#include <cstdio>
#include <thread>
#include <vector>
static bool window_by_field(unsigned bits) {
    const unsigned e = (bits >> 23) & 0xFFu;
    return e - 1u < 252u;
}
struct Part { unsigned long long differ = 0, accepted = 0; unsigned first = ~0u; };
static void run(unsigned hi0, unsigned hi1, Part* out) {
    Part p;
    for (unsigned hi = hi0; hi < hi1; hi++) {                // blocks of 2^16 patterns: counters a vectorizer can keep in lanes
        unsigned d = 0, a = 0, f = ~0u;
        for (unsigned lo = 0; lo < (1u << 16); lo++) {
            const unsigned bits = (hi << 16) | lo;
            const bool was = window_by_field(bits), is = cl2::rcp_window(bits);
            d += was != is;
            a += is;
            f = (was != is && bits < f) ? bits : f;
        }
        p.differ += d; p.accepted += a;
        p.first = f < p.first ? f : p.first;
    }
    *out = p;
}
int main() {
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned T = hw < 1 ? 1 : hw > 8 ? 8 : hw;
    std::vector<Part> parts(T);
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < T; t++)
        threads.emplace_back(run, (unsigned)((1ull << 16) * t / T), (unsigned)((1ull << 16) * (t + 1) / T), &parts[t]);
    for (auto& th : threads) th.join();
    Part all;
    for (const Part& p : parts) {
        all.differ += p.differ; all.accepted += p.accepted;
        all.first = p.first < all.first ? p.first : all.first;
    }
    const unsigned long long expected = 2ull * 252 * (1ull << 23);      // two signs x 252 exponents x 2^23 fractions
    printf("%llu of %llu patterns differ", all.differ, 1ull << 32);
    if (all.differ) printf(" (first: 0x%08x)", all.first);
    printf("; %llu accepted (expected %llu)\n", all.accepted, expected);
    return all.differ || all.accepted != expected ? 1 : 0;
}
