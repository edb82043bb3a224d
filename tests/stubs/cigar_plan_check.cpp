// Stand-alone program over rattle_amd/csrc/cigar_plan.h alone (no HIP, no device), built with -fsanitize=address,undefined by
// tests/test_cigar_plan.py: the host plan of kernel F on random and on extreme records.  Every pair with status 0 lies in exactly one
// sub-chunk, in the order given, and no other pair does; a pair needs ceil(rows / 64) * (cols + 63) code records, a strip of `cols` words
// iff it has more than one block, and rows + cols ops words; a sub-chunk holds at most pair_chunk pairs and at most code_cap code bytes
// unless it is a single pair, and is closed only when the next pair does not fit.  Prints "ok <cases>" and returns 0, or says what failed
// and returns 1.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../rattle_amd/csrc/cigar_plan.h"

using namespace rattle;

static int fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
    fprintf(stderr, "FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

typedef unsigned __int128 u128;

static int check(const std::vector<uint8_t> &status, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t pair_chunk,
                 uint64_t code_cap) {
    cigar_plan P;
    P.sub.assign(3, 99); P.first.assign(5, 99); P.recs.assign(2, 99); P.strip.assign(1, 99); P.ops.assign(4, 99);      // (a plan object is reusable)
    plan_cigar(status.data(), rows.data(), cols.data(), (uint32_t)status.size(), pair_chunk, code_cap, P);
    if (P.recs.size() != P.sub.size() || P.strip.size() != P.sub.size() || P.ops.size() != P.sub.size()) return fail("sizes");
    size_t at = 0;
    std::vector<u128> need;
    for (size_t i = 0; i < status.size(); ++i) {
        if (status[i] != 0 || !rows[i] || !cols[i]) continue;
        if (at >= P.sub.size() || P.sub[at] != i) return fail("pairs out of order", i, at);
        const u128 blocks = ((u128)rows[i] + 63) / 64, recs = blocks * ((u128)cols[i] + 63);
        if ((u128)P.recs[at] != recs) return fail("code records", i, P.recs[at]);
        if (P.strip[at] != (rows[i] > 64 ? cols[i] : 0)) return fail("strip words", i, P.strip[at]);
        if (P.ops[at] != (uint64_t)rows[i] + cols[i]) return fail("ops words", i, P.ops[at]);
        need.push_back(recs * 16);
        ++at;
    }
    if (at != P.sub.size()) return fail("more pairs than expected", at, P.sub.size());
    if (P.sub.empty()) return P.first.empty() ? 0 : fail("sub-chunks of nothing");
    if (P.first.size() < 2 || P.first.front() != 0 || P.first.back() != P.sub.size()) return fail("sub-chunk bounds");
    for (size_t c = 0; c + 1 < P.first.size(); ++c) {
        if (P.first[c] >= P.first[c + 1]) return fail("empty sub-chunk", c);
        const uint64_t n = P.first[c + 1] - P.first[c];
        u128 bytes = 0;
        for (uint32_t i = P.first[c]; i < P.first[c + 1]; ++i) bytes += need[i];
        if (n > 1 && (n > pair_chunk || bytes > code_cap)) return fail("sub-chunk over its bounds", n, (uint64_t)bytes);
        // greedy: the next pair did not fit
        if (c + 2 < P.first.size() && n < pair_chunk && bytes + need[P.first[c + 1]] <= code_cap) return fail("sub-chunk closed early", c);
    }
    return 0;
}

// the sub-chunks of a plan, as the number of pairs in each
static std::vector<uint32_t> shape(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t pair_chunk, uint64_t code_cap) {
    cigar_plan P;
    std::vector<uint8_t> status(rows.size(), 0);
    plan_cigar(status.data(), rows.data(), cols.data(), (uint32_t)rows.size(), pair_chunk, code_cap, P);
    std::vector<uint32_t> out;
    for (size_t c = 0; c + 1 < P.first.size(); ++c) out.push_back(P.first[c + 1] - P.first[c]);
    return out;
}

int main() {
    std::mt19937_64 rng(20261020);
    int cases = 0;
    for (int it = 0; it < 400; ++it) {
        const size_t n = rng() % 200;
        std::vector<uint8_t> status(n);
        std::vector<uint32_t> rows(n), cols(n);
        for (size_t i = 0; i < n; ++i) {
            status[i] = rng() % 5 == 0 ? (uint8_t)(1 + rng() % 3) : 0;
            const uint64_t k = rng() % 10;
            rows[i] = k == 0 ? 0 : k == 1 ? 63 + (uint32_t)(rng() % 4) : k == 2 ? 127 + (uint32_t)(rng() % 4) : (uint32_t)(rng() % 300);
            cols[i] = rng() % 12 == 0 ? 0 : (uint32_t)(rng() % 300);
        }
        const uint32_t pair_chunk = it % 5 == 0 ? 1 : 1 + (uint32_t)(rng() % 50);
        const uint64_t code_cap = it % 7 == 0 ? 0 : rng() % 400000;
        if (check(status, rows, cols, pair_chunk, code_cap)) return 1;
        ++cases;
    }
    // the sizes at the block's edge: 63, 64, 65, 128, 129 rows of 100 columns are 1, 1, 2, 2, 3 blocks of 163 records
    {
        cigar_plan P;
        const std::vector<uint8_t> status(5, 0);
        const std::vector<uint32_t> rows = {63, 64, 65, 128, 129}, cols(5, 100);
        plan_cigar(status.data(), rows.data(), cols.data(), 5, 8, ~0ull, P);
        const uint64_t recs[5] = {163, 163, 326, 326, 489}, strip[5] = {0, 0, 100, 100, 100};
        for (int i = 0; i < 5; ++i)
            if (P.recs[i] != recs[i] || P.strip[i] != strip[i] || P.ops[i] != rows[i] + 100ull) return fail("block edge", i, P.recs[i]);
        if (check(status, rows, cols, 8, ~0ull)) return 1;
        ++cases;
    }
    // the byte cap one below, on and above the need of two pairs of 163 records (2608 bytes each); a lone pair over the cap runs alone
    {
        const std::vector<uint32_t> rows = {64, 64, 64}, cols = {100, 100, 100};
        const uint64_t need = 163 * 16;
        if (shape(rows, cols, 8, 2 * need - 1) != std::vector<uint32_t>{1, 1, 1}) return fail("cap one below two pairs");
        if (shape(rows, cols, 8, 2 * need) != std::vector<uint32_t>{2, 1}) return fail("cap on two pairs");
        if (shape(rows, cols, 8, 2 * need + 1) != std::vector<uint32_t>{2, 1}) return fail("cap above two pairs");
        if (shape(rows, cols, 8, need - 1) != std::vector<uint32_t>{1, 1, 1}) return fail("cap below one pair");
        if (shape(rows, cols, 2, ~0ull) != std::vector<uint32_t>{2, 1}) return fail("pair_chunk");
        if (shape({10, 5000, 10, 10}, {10, 5000, 10, 10}, 8, 3 * 73 * 16) != std::vector<uint32_t>{1, 1, 2}) return fail("lone oversize pair");
        for (uint64_t cap : {2 * need - 1, 2 * need, 2 * need + 1, need - 1, (uint64_t)0})
            if (check({0, 0, 0}, rows, cols, 8, cap)) return 1;
        if (check({0, 0, 0, 0}, {10, 5000, 10, 10}, {10, 5000, 10, 10}, 8, 3 * 73 * 16)) return 1;
        cases += 6;
    }
    // statuses other than 0, alone and mixed; nothing at all
    if (check({1, 2, 3}, {5, 5, 5}, {5, 5, 5}, 4, 100) || check({3, 0, 2, 0, 1}, {0, 70, 9, 1, 0}, {0, 80, 9, 1, 0}, 1, 0) || check({}, {}, {}, 1, 1)) return 1;
    cases += 3;
    // lengths near 2^31, and beyond what the ABI lets through: nothing wraps
    const uint32_t big = (1u << 31) - 1;
    if (check({0, 0, 0}, {big, 1, big}, {big, big, 1}, 2, 1ull << 32) || check({0, 0}, {big, big}, {big, big}, 8, ~0ull) ||
        check({0}, {~0u}, {~0u}, 1, 0) || check({0, 0, 0}, {~0u, ~0u, 3}, {~0u, ~0u, 3}, 8, ~0ull))
        return 1;
    cases += 4;
    printf("ok %d\n", cases);
    return 0;
}
