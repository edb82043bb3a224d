// Stand-alone program over rattle_amd/csrc/align_plan.h alone (no HIP, no device), built with -fsanitize=address,undefined by
// tests/test_align_plan.py: the host plan of rattle_hip_align_pairs on random and on extreme lengths.  Every submitted read lies in
// exactly one chunk, in the order given; a chunk holds at most pair_chunk pairs and at most strip_cap strip records unless it is a
// single pair; a pair has a strip iff its read has more than 64 bases; the statuses follow the header's rules, max_cells without an
// overflow of Lq * Lt.  Prints "ok <cases>" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../rattle_amd/csrc/align_plan.h"

using namespace rattle;

static int fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
    fprintf(stderr, "FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

// the plan of (lengths of the targets, lengths of the reads, target of every read) against the rules, restated
static int check(const std::vector<uint64_t> &tlen, const std::vector<uint64_t> &rlen, const std::vector<int32_t> &target, uint64_t max_cells,
                 uint32_t pair_chunk, uint64_t strip_cap) {
    std::vector<uint64_t> toff(tlen.size() + 1, 1000), roff(rlen.size() + 1, 7);     // (offsets need not start at 0)
    for (size_t i = 0; i < tlen.size(); ++i) toff[i + 1] = toff[i] + tlen[i];
    for (size_t i = 0; i < rlen.size(); ++i) roff[i + 1] = roff[i] + rlen[i];
    align_plan P;
    P.sub.assign(3, 99); P.first.assign(5, 99); P.strip.assign(2, 99);             // (a plan object is reusable)
    plan_align(toff.data(), roff.data(), (uint32_t)rlen.size(), target.data(), max_cells, pair_chunk, strip_cap, P);
    if (P.status.size() != rlen.size() || P.strip.size() != P.sub.size()) return fail("sizes");
    size_t at = 0;
    for (size_t r = 0; r < rlen.size(); ++r) {
        const uint64_t lq = rlen[r], lt = target[r] < 0 ? 0 : tlen[target[r]];
        unsigned __int128 cells = (unsigned __int128)lq * lt;
        const uint8_t want = target[r] < 0 ? 3 : (lq == 0 || lt == 0) ? 1 : (max_cells && cells > max_cells) ? 2 : 0;
        if (P.status[r] != want) return fail("status", r, P.status[r]);
        if (want == 0) {
            if (at >= P.sub.size() || P.sub[at] != r) return fail("submitted reads out of order", r, at);
            if (P.strip[at] != (lq > 64 ? lt : 0)) return fail("strip records", r, P.strip[at]);
            ++at;
        }
    }
    if (at != P.sub.size()) return fail("more submitted than expected", at, P.sub.size());
    if (P.sub.empty()) return P.first.empty() ? 0 : fail("chunks of nothing");
    if (P.first.size() < 2 || P.first.front() != 0 || P.first.back() != P.sub.size()) return fail("chunk bounds");
    for (size_t c = 0; c + 1 < P.first.size(); ++c) {
        if (P.first[c] >= P.first[c + 1]) return fail("empty chunk", c);
        const uint64_t n = P.first[c + 1] - P.first[c];
        uint64_t recs = 0;
        for (uint32_t i = P.first[c]; i < P.first[c + 1]; ++i) recs += P.strip[i];
        if (n > 1 && (n > pair_chunk || recs > strip_cap)) return fail("chunk over its bounds", n, recs);
        // greedy: the next pair did not fit
        if (c + 2 < P.first.size() && n < pair_chunk && recs + P.strip[P.first[c + 1]] <= strip_cap) return fail("chunk closed early", c);
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20261019);
    int cases = 0;
    for (int it = 0; it < 400; ++it) {
        const size_t nt = 1 + rng() % 9, nr = rng() % 200;
        std::vector<uint64_t> tlen(nt), rlen(nr);
        std::vector<int32_t> target(nr);
        for (auto &l : tlen) l = rng() % 8 == 0 ? 0 : rng() % 300;
        for (auto &l : rlen) { const uint64_t k = rng() % 10; l = k == 0 ? 0 : k == 1 ? 63 + rng() % 4 : rng() % 300; }
        for (auto &t : target) t = rng() % 6 == 0 ? -1 : (int32_t)(rng() % nt);
        const uint64_t max_cells = it % 3 == 0 ? 0 : 1 + rng() % 60000;
        const uint32_t pair_chunk = it % 5 == 0 ? 1 : 1 + (uint32_t)(rng() % 50);
        const uint64_t strip_cap = it % 7 == 0 ? 0 : rng() % 3000;
        if (check(tlen, rlen, target, max_cells, pair_chunk, strip_cap)) return 1;
        ++cases;
    }
    // the edge of max_cells, one below and on Lq * Lt, and lengths whose product does not fit 64 bits
    if (check({30}, {24, 24}, {0, 0}, 24 * 30 - 1, 4, 100) || check({30}, {24, 24}, {0, 0}, 24 * 30, 4, 100)) return 1;
    const uint64_t big = (1ull << 31) - 1;
    if (check({big, 5}, {big, big, 3}, {0, 1, 0}, ~0ull, 2, 1ull << 26) || check({big}, {big}, {0}, 0, 1, 0)) return 1;
    if (check({1ull << 40}, {1ull << 40, 1}, {0, 0}, 1ull << 63, 8, 5)) return 1;
    if (check({}, {}, {}, 0, 1, 1) || check({4}, {4, 4}, {-1, -1}, 0, 1, 1)) return 1;
    cases += 7;
    printf("ok %d\n", cases);
    return 0;
}
