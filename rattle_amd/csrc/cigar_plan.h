// The host plan of kernel F (pair_cigar.hip) for one chunk of kernel E: which pairs go on to the traceback, how many code records, strip
// words and ops words each needs, and how they fall into sub-chunks -- from kernel E's statuses and the two spans of every record alone.
// Pure host code, no HIP: tests/stubs/cigar_plan_check.cpp builds this header alone, under the sanitizers.
//
// A pair's rectangle has `rows` = q_end - q_start rows and `cols` = t_end - t_start columns.  Kernel F takes the rows in blocks of 64 and
// writes one 16-byte code record per (block, step); a block's records lie `cols + 63` apart whatever its height, so a pair needs
//   blocks * (cols + 63) records,  blocks = ceil(rows / 64)
// a hand-over strip of `cols` 4-byte words if it has more than one block, and an ops region of rows + cols words (every column a run of its
// own).  The lengths are below 2^31 (the ABI refuses longer sequences), so none of these overflows 64 bits; the one product is formed by
// cg_mul, which saturates, and sums saturate too: a plan over absurd lengths is a plan whose allocation fails, never a short buffer.
#pragma once
#include <stdint.h>

#include <vector>

namespace rattle {

constexpr uint32_t CG_ROWS = 64;                 // rows of a block of kernel F = lanes of a wavefront
constexpr uint64_t CG_REC_BYTES = 16;            // one code record: two 64-bit ballots
constexpr uint64_t CG_AFFINE_REC_BYTES = 32;     // ... of the three-state form: four ballots
constexpr uint64_t CG_AFFINE_STRIP_WORDS = 2;    // ... and its strip holds H and U of every column
constexpr uint64_t CG_CODE_CAP = 1ull << 32;     // default cap on a sub-chunk's code bytes: 4 GiB

inline uint64_t cg_mul(uint64_t a, uint64_t b) { return a && b > ~0ull / a ? ~0ull : a * b; }
inline uint64_t cg_add(uint64_t a, uint64_t b) { return a > ~0ull - b ? ~0ull : a + b; }

struct cigar_plan {
    std::vector<uint32_t> sub;                   // the pairs of the chunk that go on (status 0 and a rectangle that is not empty), in order
    std::vector<uint64_t> recs;                  // [sub.size()] code records
    std::vector<uint64_t> strip;                 // [sub.size()] strip words: cols if the rectangle has more than one block, else 0
    std::vector<uint64_t> ops;                   // [sub.size()] words of the ops region: rows + cols
    std::vector<uint32_t> first;                 // sub-chunk c = sub[first[c] .. first[c + 1]); empty if nothing goes on
};

// A sub-chunk holds at most pair_chunk pairs and at most code_cap bytes of code records; one pair always fits, whatever it needs (a pair that
// alone exceeds the cap runs alone: its allocation succeeds or the call ends with the library's out-of-memory error).
// rec_bytes, strip_words: the bytes of one code record and the strip's words per column -- 16 and 1 for kernel F, 32 and 2 for its
// three-state form (pair_cigar_kernel<true>: four bits per cell, H and U in the strip); pair_wave.h names both sets as a gap_form.
inline void plan_cigar(const uint8_t *status, const uint32_t *rows, const uint32_t *cols, uint32_t n, uint32_t pair_chunk, uint64_t code_cap,
                       cigar_plan &P, uint64_t rec_bytes = CG_REC_BYTES, uint64_t strip_words = 1) {
    P.sub.clear(); P.recs.clear(); P.strip.clear(); P.ops.clear(); P.first.clear();
    for (uint32_t i = 0; i < n; ++i) {
        if (status[i] != 0 || rows[i] == 0 || cols[i] == 0) continue;
        const uint64_t blocks = ((uint64_t)rows[i] + CG_ROWS - 1) / CG_ROWS;
        P.sub.push_back(i);
        P.recs.push_back(cg_mul(blocks, (uint64_t)cols[i] + CG_ROWS - 1));
        P.strip.push_back(blocks > 1 ? cg_mul(cols[i], strip_words) : 0);
        P.ops.push_back((uint64_t)rows[i] + cols[i]);
    }
    if (P.sub.empty()) return;
    P.first.push_back(0);
    uint64_t pairs = 0, bytes = 0;
    for (size_t i = 0; i < P.sub.size(); ++i) {
        const uint64_t need = cg_mul(P.recs[i], rec_bytes);
        if (pairs && (pairs >= pair_chunk || cg_add(bytes, need) > code_cap)) { P.first.push_back((uint32_t)i); pairs = 0; bytes = 0; }
        ++pairs; bytes = cg_add(bytes, need);
    }
    P.first.push_back((uint32_t)P.sub.size());
}

}  // namespace rattle
