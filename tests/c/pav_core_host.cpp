// Host replay of the PAV hull kernels: includes csrc/nplda_pav_core.h and runs binning flags, the chunk scan and the
// whole merge tree serially, exactly as csrc/nplda_pav.hip schedules them (same buffers, same index arithmetic), with
// chunk lengths 2, 3, 4 and 8 so that tiny inputs build deep trees.  Every vertex list is compared with the O(n) stack
// over ALL bin points.  Exit status 0 iff nothing differs.  Built with -fsanitize=address,undefined by
// tests/test_pav_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../neuralplda_amd/csrc/nplda_pav_core.h"

namespace {

struct Bin {
    uint32_t n, t;
};

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// O(n) reference: strict lower hull of P_0 .. P_M
std::vector<PavPt> stack_hull(const std::vector<PavPt>& p) {
    std::vector<PavPt> h;
    for (const PavPt& c : p) {
        while (h.size() >= 2) {
            const PavPt a = h[h.size() - 2], b = h[h.size() - 1];
            const __int128 cr = (__int128)((int64_t)b.x - a.x) * ((int64_t)c.y - b.y) -
                                (__int128)((int64_t)b.y - a.y) * ((int64_t)c.x - b.x);
            if (cr > 0) break;
            h.pop_back();
        }
        h.push_back(c);
    }
    return h;
}

std::vector<Bin> family(int f, int N) {
    std::vector<Bin> b;
    switch (f) {
    case 0:  // perfectly separated, distinct scores
        for (int i = 0; i < N; ++i) b.push_back({1u, i >= N / 2 ? 1u : 0u});
        break;
    case 1:  // perfectly inverted
        for (int i = 0; i < N; ++i) b.push_back({1u, i < N / 2 ? 1u : 0u});
        break;
    case 2:  // all tied
        b.push_back({(uint32_t)N, (uint32_t)(N / 3)});
        break;
    case 3:  // strictly alternating
        for (int i = 0; i < N; ++i) b.push_back({1u, (uint32_t)(i & 1)});
        break;
    case 4:  // staircase: n = m + 1, t = 1 .. m
        for (int k = 1; k <= N; ++k) b.push_back({(uint32_t)N + 1, (uint32_t)k});
        break;
    case 5:  // reversed staircase
        for (int k = N; k >= 1; --k) b.push_back({(uint32_t)N + 1, (uint32_t)k});
        break;
    case 6:  // every cross product is 0
        for (int i = 0; i < N; ++i) b.push_back({2u, 1u});
        break;
    case 7:  // heavy all-target bin on the far left, then a staircase
        b.push_back({(uint32_t)(N * N + 7), (uint32_t)(N * N + 7)});
        for (int k = 1; k <= N; ++k) b.push_back({(uint32_t)N + 1, (uint32_t)k});
        break;
    case 8:  // 10 % targets, distinct scores, the targets more likely on the right
        for (int i = 0; i < N; ++i) b.push_back({1u, (rnd() % 1000) < (uint32_t)(20 + 160 * i / (N > 1 ? N : 1)) ? 1u : 0u});
        break;
    case 9:  // heavy ties: random bins
        for (int i = 0; i < N; ++i) {
            const uint32_t n = 1 + rnd() % 5;
            b.push_back({n, rnd() % (n + 1)});
        }
        break;
    case 10:  // heavy anchor on the right (mirror of 7): one all-non-target bin last
        for (int k = 1; k <= N; ++k) b.push_back({(uint32_t)N + 1, (uint32_t)k});
        b.push_back({(uint32_t)(N * N + 7), 0u});
        break;
    default:  // a convex run followed by a concave one and noise
        for (int i = 0; i < N; ++i) {
            const uint32_t n = 4 + (uint32_t)(i % 3);
            const int up = i < N / 2 ? i : N - i;
            b.push_back({n + (uint32_t)N, (uint32_t)(up % (int)(n + N)) + rnd() % 2});
        }
        break;
    }
    return b;
}
const int kFamilies = 12;

int failures = 0;

void run_case(int f, int N, int C, int laplace, int filter) {
    const std::vector<Bin> bins = family(f, N);
    // every bin point, the dummy bins of the Laplace rule included: the reference hull
    std::vector<PavPt> all;
    all.push_back({0u, 0u});
    uint32_t x = 0, y = 0;
    if (laplace) all.push_back({x += 2, y += 1});
    for (const Bin& b : bins) all.push_back({x += b.n, y += b.t});
    if (laplace) all.push_back({x += 2, y += 1});
    const std::vector<PavPt> want = stack_hull(all);

    // sorted trials as the kernels see them: key = the bin's number, labels in a mixed order inside a bin
    std::vector<double> key;
    std::vector<uint64_t> lab, pref;
    for (size_t k = 0; k < bins.size(); ++k) {
        uint32_t t = bins[k].t, n = bins[k].n - bins[k].t;
        while (t + n) {
            const bool tgt = n == 0 || (t > 0 && (rnd() & 1));
            key.push_back(k == 0 ? -0.0 : (double)k * 0.5);
            lab.push_back(tgt ? 1ull << 32 : 1ull);
            if (tgt) --t; else --n;
        }
    }
    const int64_t nk = (int64_t)key.size();
    uint64_t acc = 0;
    for (int64_t i = 0; i < nk; ++i) {
        pref.push_back(acc);
        acc += lab[i];
    }
    // flag + scan + compaction (the point kernel)
    const uint32_t off = laplace ? 2u : 0u, yoff = laplace ? 1u : 0u;
    const int64_t maxpts = nk + 4;
    std::vector<PavPt> A((size_t)maxpts, PavPt{0xdeadbeefu, 0xdeadbeefu}), B((size_t)maxpts, PavPt{0xdeadbeefu, 0xdeadbeefu});
    int64_t m = 0;
    A[m++] = {0u, 0u};
    if (laplace) A[m++] = {2u, 1u};
    int64_t M = 0;
    for (int64_t i = 0; i < nk; ++i) {
        const uint64_t fl = pav_flag(key.data(), lab.data(), pref.data(), nk, i, filter);
        M += (int64_t)(fl >> 32);
        if (fl & 1ull) A[m++] = {(uint32_t)(i + 1) + off, (uint32_t)((pref[i] + lab[i]) >> 32) + yoff};
    }
    if (laplace) A[m++] = {(uint32_t)nk + 4u, (uint32_t)(acc >> 32) + 2u};
    if (M != (int64_t)bins.size()) {
        std::printf("FAIL bins f=%d N=%d: %lld != %zu\n", f, N, (long long)M, bins.size());
        ++failures;
    }
    // level 0
    const int64_t chunks = pav_hulls(maxpts, C, 0);
    std::vector<int32_t> cntA((size_t)chunks, 0), cntB((size_t)chunks, 0);
    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t b0 = c * C;
        const int64_t n = b0 >= m ? 0 : (m - b0 < C ? m - b0 : C);
        cntA[(size_t)c] = n > 0 ? pav_chunk_scan(A.data() + b0, (int)n) : 0;
    }
    // merge levels: launch count from maxpts alone
    const int levels = pav_levels(maxpts, C);
    PavPt *src = A.data(), *dst = B.data();
    int32_t *csrc = cntA.data(), *cdst = cntB.data();
    for (int L = 1; L <= levels; ++L) {
        const int64_t span = pav_span(C, L), half = span >> 1;
        const int64_t groups = pav_hulls(maxpts, C, L), nsrc = pav_hulls(maxpts, C, L - 1);
        std::vector<PavBridge> br((size_t)groups);
        for (int64_t g = 0; g < groups; ++g) {
            const int kl = csrc[2 * g];
            const int kr = 2 * g + 1 < nsrc ? csrc[2 * g + 1] : 0;
            br[(size_t)g] = pav_bridge(src + g * span, kl, src + g * span + half, kr);
            cdst[g] = pav_merged_count(br[(size_t)g]);
        }
        for (int64_t p = 0; p < m; ++p) {
            const int64_t g = p / span, e = p - g * span;
            const int64_t s = pav_merged_src(br[(size_t)g], span, e);
            if (s >= 0) dst[p] = src[g * span + s];
        }
        PavPt* tp = src; src = dst; dst = tp;
        int32_t* tc = csrc; csrc = cdst; cdst = tc;
    }
    const int got = csrc[0];
    bool ok = got == (int)want.size();
    for (int i = 0; ok && i < got; ++i) ok = src[i].x == want[(size_t)i].x && src[i].y == want[(size_t)i].y;
    if (!ok) {
        if (failures < 20) {
            std::printf("FAIL f=%d N=%d C=%d laplace=%d filter=%d: got %d vertices, want %zu\n", f, N, C, laplace, filter, got,
                        want.size());
        }
        ++failures;
    }
}

}  // namespace

int main() {
    const int Cs[] = {2, 3, 4, 8};
    long cases = 0;
    for (int f = 0; f < kFamilies; ++f)
        for (int N = 1; N <= 200; ++N) {
            // the families of N bins with N + 1 trials each grow as N^2: above N = 48 they rotate through the
            // (C, laplace, filter) combinations instead of running all sixteen
            const bool heavy = (f == 4 || f == 5 || f == 7 || f == 10 || f == 11) && N > 48;
            int combo = 0;
            for (int C : Cs)
                for (int lap = 0; lap < 2; ++lap)
                    for (int filt = 0; filt < 2; ++filt, ++combo) {
                        if (heavy && combo != (N + f) % 16) continue;
                        run_case(f, N, C, lap, filt);
                        ++cases;
                    }
        }
    std::printf("%ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
