// What kernels E and F (pair_align.hip, pair_cigar.hip) share: the two forms of each as the host sees them, and the device helpers of the
// skewed one-wavefront-per-pair form -- lane l owns row 64 b + l of block b, at step s it computes column s - l; what crosses a row comes
// from lane l - 1 by pw_shr1, lane 0's from the pair's hand-over strip, which is read one refill (64 columns) ahead and updated in place
// behind the reads.  pair_align.hip describes the shape in full.
#pragma once
#include "align_plan.h"
#include "cigar_plan.h"
#include "common.h"

namespace rattle {

// Each kernel is one template in two forms: <false> linear gaps at 5,4,8,8, <true> affine gaps with the caller's scoring, three states per
// cell.  The second template argument, the mode (local, or the whole read: RATTLE_ALIGN_READ), changes neither the ids nor the layouts.
// What the host has to know of a form:
struct gap_form {
    int k_align, k_cigar;               // ids of the kernel stats
    uint64_t strip_bytes;               // kernel E: bytes of the hand-over strip per column
    uint64_t rec_bytes, strip_words;    // kernel F: bytes of a code record, words of the strip per column
};
constexpr gap_form GAP_LINEAR = {K_ALIGN, K_CIGAR, AL_STRIP_BYTES, CG_REC_BYTES, 1};
constexpr gap_form GAP_AFFINE = {K_ALIGN_AFFINE, K_CIGAR_AFFINE, AL_AFFINE_STRIP_BYTES, CG_AFFINE_REC_BYTES, CG_AFFINE_STRIP_WORDS};

constexpr rattle_align_scoring PW_LINEAR = {5, 4, 8, 8};       // the scoring of the linear form: a gap column costs 8, opened or extended
// Minus infinity of a gap state.  It is never decremented twice: a gap state that is kept is max(H - o, state - e) >= H - o of a cell on the
// matrix or its border, and every such H is >= 0 (local) or >= -(o + e (Lq - 1)) > -2^29 (read mode: H >= U >= the gap straight down from
// row 0; abi.hip keeps that below 2^29).  So with o, e <= 64 every kept U is > -2^29 and every kept L > -2^29 - 64, both above PW_NEG, whose
// own open or extend, PW_NEG - 64, does not wrap and loses every max.
constexpr int32_t PW_NEG = -(1 << 30);
constexpr uint32_t PW_OP_I = 1, PW_OP_D = 2, PW_OP_EQ = 7, PW_OP_X = 8;      // BAM's numbers
constexpr uint32_t PW_MAX_RUN = 0x0FFFFFFFu;                   // 28 bits of length: a longer run is written in pieces

// value of lane - 1 (lane 0 receives `fill`): the helper of poa.hip
__device__ __forceinline__ int32_t pw_shr1(int32_t v, int32_t fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
}

// A 0, C 1, G 2, T and U 3 (the complement of code c is 3 - c); the host has refused every other byte
__device__ __forceinline__ int32_t pw_code(uint32_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3; }

__device__ __forceinline__ uint32_t pw_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v); }

}  // namespace rattle
