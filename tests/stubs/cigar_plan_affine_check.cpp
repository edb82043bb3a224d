// Stand-alone program over rattle_amd/csrc/cigar_plan.h alone (no HIP, no device), built with -fsanitize=address,undefined by
// tests/test_align_affine_plan.py: the host plan of the three-state kernel F -- 32-byte code records, two strip words per column (H and U)
// -- against counts written out by hand, the saturating products, and the plan of the old signature, which must be what it was.  Prints
// "ok <cases>" and returns 0, or says what failed and returns 1.
#include <cstdio>

#include "../../rattle_amd/csrc/cigar_plan.h"

using namespace rattle;

static int fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
    fprintf(stderr, "FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

static std::vector<uint32_t> shape(const cigar_plan &P) {
    std::vector<uint32_t> out;
    for (size_t c = 0; c + 1 < P.first.size(); ++c) out.push_back(P.first[c + 1] - P.first[c]);
    return out;
}

int main() {
    int cases = 0;
    if (CG_AFFINE_REC_BYTES != 32 || CG_AFFINE_STRIP_WORDS != 2 || CG_REC_BYTES != 16) return fail("constants");
    // 63, 64, 65, 128, 129 rows of 100 columns are 1, 1, 2, 2, 3 blocks of 163 records: the records are counted as before, the strip
    // has 2 words per column from two blocks on, the ops region is rows + cols words; a pair with status 1 and an empty rectangle drop out
    {
        const std::vector<uint8_t> status = {0, 0, 1, 0, 0, 0, 0};
        const std::vector<uint32_t> rows = {63, 64, 70, 65, 128, 0, 129}, cols = {100, 100, 100, 100, 100, 100, 100};
        cigar_plan P;
        plan_cigar(status.data(), rows.data(), cols.data(), 7, 8, ~0ull, P, 32, 2);
        const uint32_t sub[5] = {0, 1, 3, 4, 6};
        const uint64_t recs[5] = {163, 163, 326, 326, 489}, strip[5] = {0, 0, 200, 200, 200}, ops[5] = {163, 164, 165, 228, 229};
        if (P.sub.size() != 5 || P.recs.size() != 5 || P.strip.size() != 5 || P.ops.size() != 5) return fail("sizes", P.sub.size());
        for (int i = 0; i < 5; ++i)
            if (P.sub[i] != sub[i] || P.recs[i] != recs[i] || P.strip[i] != strip[i] || P.ops[i] != ops[i]) return fail("block edge", i, P.strip[i]);
        if (shape(P) != std::vector<uint32_t>{5}) return fail("one sub-chunk");
        ++cases;
    }
    // the byte cap one below, on and above the need of two pairs of 163 records at 32 bytes (5216 each); under the same caps the 16-byte
    // plan holds twice the pairs; a lone pair over the cap runs alone; pair_chunk
    {
        const std::vector<uint8_t> status(4, 0);
        const std::vector<uint32_t> rows(4, 64), cols(4, 100);
        const uint64_t need = 163 * 32;
        auto plan = [&](uint32_t chunk, uint64_t cap, uint64_t rec_bytes) {
            cigar_plan P;
            plan_cigar(status.data(), rows.data(), cols.data(), 4, chunk, cap, P, rec_bytes, rec_bytes == 32 ? 2 : 1);
            return shape(P);
        };
        if (need != 5216) return fail("need");
        if (plan(8, 2 * need - 1, 32) != std::vector<uint32_t>{1, 1, 1, 1}) return fail("cap one below two pairs");
        if (plan(8, 2 * need, 32) != std::vector<uint32_t>{2, 2}) return fail("cap on two pairs");
        if (plan(8, 2 * need + 1, 32) != std::vector<uint32_t>{2, 2}) return fail("cap above two pairs");
        if (plan(8, 3 * need, 32) != std::vector<uint32_t>{3, 1}) return fail("cap on three pairs");
        if (plan(8, 2 * need, 16) != std::vector<uint32_t>{4}) return fail("16-byte records under the cap of two 32-byte pairs");
        if (plan(8, need - 1, 32) != std::vector<uint32_t>{1, 1, 1, 1}) return fail("cap below one pair");
        if (plan(3, ~0ull, 32) != std::vector<uint32_t>{3, 1}) return fail("pair_chunk");
        cases += 7;
    }
    // the old signature gives the old plan: field for field that of (16, 1), and a strip of `cols` words
    {
        const std::vector<uint8_t> status = {0, 2, 0, 0, 3, 0};
        const std::vector<uint32_t> rows = {200, 5, 64, 65, 9, 1}, cols = {700, 5, 1, 300, 9, 1};
        cigar_plan A, B, C;
        plan_cigar(status.data(), rows.data(), cols.data(), 6, 2, 40000, A);
        plan_cigar(status.data(), rows.data(), cols.data(), 6, 2, 40000, B, 16, 1);
        plan_cigar(status.data(), rows.data(), cols.data(), 6, 2, 40000, C, 32, 2);
        if (A.sub != B.sub || A.recs != B.recs || A.strip != B.strip || A.ops != B.ops || A.first != B.first) return fail("old signature");
        const uint64_t recs[4] = {4 * 763, 64, 2 * 363, 64}, strip[4] = {700, 0, 300, 0};
        for (int i = 0; i < 4; ++i) if (A.recs[i] != recs[i] || A.strip[i] != strip[i]) return fail("old plan", i);
        // 48832 bytes alone, then 1024 + 11616, then 1024: under 40000 the first pair runs alone
        if (shape(A) != std::vector<uint32_t>{1, 2, 1}) return fail("old sub-chunks");
        // 32-byte records: 97664 alone, 2048 + 23232 = 25280, 2048 (pair_chunk 2 closes the second)
        if (C.sub != A.sub || C.recs != A.recs || C.ops != A.ops || C.strip != std::vector<uint64_t>{1400, 0, 600, 0}) return fail("new plan");
        if (shape(C) != std::vector<uint32_t>{1, 2, 1}) return fail("new sub-chunks");
        cases += 2;
    }
    // the saturating products: lengths the ABI would refuse do not wrap, in records, in bytes or in strip words
    {
        const uint32_t big = ~0u;
        const std::vector<uint8_t> status = {0, 0, 0};
        const std::vector<uint32_t> rows = {big, big, 3}, cols = {big, big, 3};
        cigar_plan P;
        plan_cigar(status.data(), rows.data(), cols.data(), 3, 8, ~0ull - 1, P, 32, 2);
        const uint64_t blocks = ((uint64_t)big + 63) / 64, recs = blocks * ((uint64_t)big + 63);      // 2^26 * (2^32 + 62): fits 64 bits
        if (P.recs[0] != recs || P.strip[0] != 2ull * big || P.ops[0] != 2ull * big) return fail("large pair", P.recs[0], P.strip[0]);
        if (cg_mul(recs, 32) != recs * 32 || cg_mul(recs, 1ull << 40) != ~0ull || cg_mul(0, ~0ull) != 0 || cg_mul(~0ull, 2) != ~0ull) return fail("cg_mul");
        if (cg_add(~0ull - 1, 1) != ~0ull || cg_add(~0ull, 5) != ~0ull || cg_add(3, 4) != 7) return fail("cg_add");
        if (shape(P) != std::vector<uint32_t>{1, 2}) return fail("a saturating sum closes the sub-chunk");      // 2 * recs * 32 > 2^64 - 1 > the cap
        cigar_plan Q;
        plan_cigar(status.data(), rows.data(), cols.data(), 3, 8, ~0ull - 1, Q, ~0ull, ~0ull);                // absurd parameters saturate as well
        if (Q.strip[0] != ~0ull || shape(Q) != std::vector<uint32_t>{1, 1, 1}) return fail("saturating parameters");
        cases += 2;
    }
    printf("ok %d\n", cases);
    return 0;
}
