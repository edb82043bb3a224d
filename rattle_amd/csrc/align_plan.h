// The host plan of rattle_hip_align_pairs (pair_align.hip): which reads go to the device, what the others' status is, how many strip
// records each submitted pair needs and how the pairs fall into chunks -- from offsets and indices alone.  Pure host code, no HIP:
// tests/stubs/align_plan_check.cpp builds this header alone, under the sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

namespace rattle {

constexpr uint32_t AL_ROWS = 64;                 // rows of a block of kernel E = lanes of a wavefront
constexpr uint64_t AL_STRIP_BYTES = 16;          // a column of the hand-over strip: H's score and its three payload words
constexpr uint64_t AL_AFFINE_STRIP_BYTES = 40;   // ... of the three-state form: H and U, a score and four payload words each

struct align_plan {
    std::vector<uint8_t> status;                 // [n_reads] 1, 2, 3 as in rattle_alignment; 0: submitted, the device decides between 0 and 1
    std::vector<uint32_t> sub;                   // the submitted reads, in the order given
    std::vector<uint64_t> strip;                 // [sub.size()] records of the pair's hand-over strip: Lt if the read has more than one block, else 0
    std::vector<uint32_t> first;                 // chunk c = sub[first[c] .. first[c + 1]); empty if nothing is submitted
};

// The arguments have been checked (every target index < n_targets or < 0).  A chunk holds at most pair_chunk pairs and at most strip_cap
// strip records; one pair always fits, whatever its strip.
inline void plan_align(const uint64_t *toff, const uint64_t *roff, uint32_t n_reads, const int32_t *target, uint64_t max_cells, uint32_t pair_chunk,
                       uint64_t strip_cap, align_plan &P) {
    P.status.assign(n_reads, 0);
    P.sub.clear(); P.strip.clear(); P.first.clear();
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (target[r] < 0) { P.status[r] = 3; continue; }
        const uint64_t lq = roff[r + 1] - roff[r], lt = toff[target[r] + 1] - toff[target[r]];
        if (lq == 0 || lt == 0) { P.status[r] = 1; continue; }
        if (max_cells && lq > max_cells / lt) { P.status[r] = 2; continue; }      // lq * lt > max_cells, without forming the product
        P.sub.push_back(r);
        P.strip.push_back(lq > AL_ROWS ? lt : 0);
    }
    if (P.sub.empty()) return;
    P.first.push_back(0);
    uint64_t pairs = 0, recs = 0;
    for (size_t i = 0; i < P.sub.size(); ++i) {
        if (pairs && (pairs >= pair_chunk || recs + P.strip[i] > strip_cap)) { P.first.push_back((uint32_t)i); pairs = 0; recs = 0; }
        ++pairs; recs += P.strip[i];
    }
    P.first.push_back((uint32_t)P.sub.size());
}

}  // namespace rattle
