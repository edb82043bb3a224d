// The byte strings the ranks of one job send each other (exchange.hip), written and read in one place.
//
// A piece arrives from outside the program -- a caller's all-gather-v, an RCCL peer, a record file -- so nothing in it is believed:
// wire_reader hands out a view of an array only if its bytes are there and aligned, and every parser checks the counts, offsets and
// ids of its format against what the receiver already knows.  A parser returns false and leaves the reason in the reader; it never
// reads beyond the piece and copies nothing (the root of a `correct` job merges views of gigabytes).
//
// Plain C++17 over the public header: no HIP here, so the parsers can be built and run under a sanitizer on their own
// (tests/stubs/wire_check.cpp).  DESIGN.md, "What the ranks exchange", lists the four payloads field by field.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rattle_hip.h"

namespace rattle {

// appends to a byte string
struct wire_writer {
    std::vector<uint8_t> &b;
    explicit wire_writer(std::vector<uint8_t> &out) : b(out) {}
    void reserve(size_t more) { b.reserve(b.size() + more); }      // one growth for what follows, not a doubling per array
    template <typename T>
    void put(const T *p, size_t n) {
        // (insert, not resize + memcpy: a resize zero-fills what the copy then overwrites -- 0.16 s of a rank's 250 MB piece at eight ranks)
        if (n) b.insert(b.end(), (const uint8_t *)p, (const uint8_t *)p + n * sizeof(T));
    }
    template <typename T>
    void put1(const T &v) { put(&v, 1); }
    void zeros(size_t n) { const uint8_t z[8] = {0}; put(z, n); }      // padding, n <= 8
};

// reads a piece front to back.  The first failed read stays: every later read fails too, so a parser may read a run of fields and
// test ok() once.  (A view of zero entries is whatever address the reader stands at, null for an empty piece: test ok(), not the pointer.)
class wire_reader {
    const uint8_t *p;
    size_t n, at = 0;
    const char *why = nullptr;

  public:
    wire_reader(const uint8_t *data, size_t bytes) : p(data), n(bytes) {}
    bool ok() const { return why == nullptr; }
    const char *reason() const { return why ? why : "no error"; }
    bool fail(const char *reason) { if (!why) why = reason; return false; }
    size_t remaining() const { return n - at; }
    bool done() const { return ok() && at == n; }
    // a view of count entries of T, or null
    template <typename T>
    const T *take(uint64_t count) {
        if (why) return nullptr;
        if (count > (n - at) / sizeof(T)) { fail("the piece ends inside an array"); return nullptr; }      // (no product: it cannot overflow)
        const uint8_t *q = p + at;
        if ((uintptr_t)q % alignof(T)) { fail("an array is not aligned for its type"); return nullptr; }
        at += (size_t)count * sizeof(T);
        return (const T *)q;
    }
    // a scalar at any address
    template <typename T>
    bool read(T &v) {
        if (why) return false;
        if (sizeof(T) > n - at) return fail("the piece ends inside a field");
        memcpy(&v, p + at, sizeof(T));
        at += sizeof(T);
        return true;
    }
    bool skip(uint64_t bytes) {
        if (why) return false;
        if (bytes > n - at) return fail("the piece ends inside its padding");
        at += (size_t)bytes;
        return true;
    }
};

// "<exchange point>: malformed piece from rank <r>: <reason>"
inline std::string wire_error(const char *point, int rank, const wire_reader &R) {
    return std::string(point) + ": malformed piece from rank " + std::to_string(rank) + ": " + R.reason();
}

// [0] = 0, non-decreasing
inline bool wire_offsets_ok(const uint64_t *off, uint64_t n) {
    if (off[0] != 0) return false;
    for (uint64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return false;
    return true;
}

// ---- 1. the gather of a sharded correction: what a rank that is not the root sends to it -------------------------------------------
// Two read sets (corrected, uncorrected), the skip list, the eight counters, the correction report of the corrected records if the
// rank made one.  8-byte fields come first in every part and every part is padded to 8 bytes: each array is naturally aligned.
enum { WIRE_REP_FIELDS = 10 };           // == REP_FIELDS (common.h)

struct piece_view {                      // one rank's read set, with the pack of every record
    uint32_t n = 0;
    const int32_t *read_id = nullptr, *cluster_id = nullptr, *n_reads = nullptr;
    const uint32_t *pack = nullptr;
    const uint64_t *off = nullptr;
    const char *seq = nullptr, *qual = nullptr;
    const uint32_t *rep[WIRE_REP_FIELDS] = {};      // the correction report of the records (corrected set), if the rank made one
    bool has_rep = false;
};
struct skip_view {
    uint64_t n = 0;
    const uint64_t *read_off = nullptr;
    const int32_t *cluster_id = nullptr;
    const uint32_t *pack = nullptr, *stage = nullptr;
    const int32_t *read_id = nullptr;
};
struct gather_view {
    piece_view corrected, uncorrected;
    skip_view skipped;
    const uint64_t *counters = nullptr;  // [8]
};

inline void write_read_set(std::vector<uint8_t> &b, const rattle_read_set &S, const uint32_t *pack) {
    wire_writer W(b);
    const uint64_t n = S.n, tot = S.off[n];
    W.reserve(16 + (n + 1) * 8 + n * 16 + 2 * tot + 8);
    W.put1(n);
    W.put(S.off, n + 1);
    W.put(S.read_id, n); W.put(S.cluster_id, n); W.put(S.n_reads, n);
    std::vector<uint32_t> none;
    if (!pack) { none.assign(n, 0); pack = none.data(); }
    W.put(pack, n);                      // 4 x 4n bytes: still 8-byte aligned
    W.put(S.seq, tot); W.put(S.qual, tot);
    W.zeros((8 - (2 * tot) % 8) % 8);
}

// rep: the WIRE_REP_FIELDS arrays of L.corrected.n entries, or null if the rank made no report
inline void write_gather_piece(std::vector<uint8_t> &b, const rattle_correction &L, uint32_t *const *rep) {
    write_read_set(b, L.corrected, L.corrected_pack);
    write_read_set(b, L.uncorrected, L.uncorrected_pack);
    wire_writer W(b);
    const rattle_skip_list &K = L.skipped;
    const uint64_t n = K.n, tot = K.read_off[K.n];
    W.put1(n); W.put(K.read_off, n + 1);
    W.put(K.cluster_id, n); W.put(K.pack, n); W.put(K.stage, n); W.put(K.read_id, tot);
    if ((3 * n + tot) & 1) W.put1((uint32_t)0);
    W.put(L.counters, 8);
    const uint64_t has = rep ? 1 : 0;
    W.put1(has);
    if (has) for (int f = 0; f < WIRE_REP_FIELDS; ++f) W.put(rep[f], L.corrected.n);      // ten arrays of 4-byte entries: 8-byte aligned as a whole
}

inline bool parse_read_set(wire_reader &R, piece_view &V) {
    uint64_t n = 0;
    if (!R.read(n)) return false;
    if (n > 0xFFFFFFFFull || n >= R.remaining() / 8) return R.fail("a read set's record count exceeds the piece");
    V.n = (uint32_t)n;
    V.off = R.take<uint64_t>(n + 1);
    V.read_id = R.take<int32_t>(n); V.cluster_id = R.take<int32_t>(n); V.n_reads = R.take<int32_t>(n);
    V.pack = R.take<uint32_t>(n);
    if (!R.ok()) return false;
    if (!wire_offsets_ok(V.off, n)) return R.fail("a read set's offsets do not start at 0 or decrease");
    const uint64_t tot = V.off[n];
    if (tot > R.remaining() / 2) return R.fail("a read set's offsets end beyond the piece");
    V.seq = R.take<char>(tot); V.qual = R.take<char>(tot);
    return R.skip((8 - (2 * tot) % 8) % 8);
}

// the whole piece, consumed to its last byte
inline bool parse_gather_piece(wire_reader &R, gather_view &G) {
    if (!parse_read_set(R, G.corrected) || !parse_read_set(R, G.uncorrected)) return false;
    skip_view &K = G.skipped;
    if (!R.read(K.n)) return false;
    if (K.n >= R.remaining() / 8) return R.fail("the skip list's entry count exceeds the piece");
    K.read_off = R.take<uint64_t>(K.n + 1);
    K.cluster_id = R.take<int32_t>(K.n); K.pack = R.take<uint32_t>(K.n); K.stage = R.take<uint32_t>(K.n);
    if (!R.ok()) return false;
    if (!wire_offsets_ok(K.read_off, K.n)) return R.fail("the skip list's offsets do not start at 0 or decrease");
    const uint64_t tot = K.read_off[K.n];
    K.read_id = R.take<int32_t>(tot);
    if ((3 * K.n + tot) & 1) R.skip(4);
    G.counters = R.take<uint64_t>(8);
    uint64_t has = 0;
    if (!R.read(has)) return false;
    if (has > 1) return R.fail("the report flag is neither 0 nor 1");
    G.corrected.has_rep = has != 0;
    if (has) for (int f = 0; f < WIRE_REP_FIELDS; ++f) G.corrected.rep[f] = R.take<uint32_t>(G.corrected.n);
    if (!R.ok()) return false;
    return R.done() || R.fail("bytes behind the end of the piece");
}

// ---- 2. the stage records of `correct`: pack consensi (kind 0) and cluster consensi (kind 1), dead flags included ----------------------
// Records [u32 id][u32 flag][u32 len][len bytes] back to back, no count in front and no padding (fields at any address).
// flag: bit 0 the kind, the bits above it why the pack or cluster has no consensus (0: it has one, the len bytes).
// A rank that has failed sends the one record (0xFFFFFFFF, 0xFFFFFFFF, 0) instead.
struct stage_rec {
    uint32_t id = 0, flag = 0, len = 0;
    const char *s = nullptr;
    uint32_t kind() const { return flag & 1u; }
    uint32_t dead() const { return flag >> 1; }
};

inline void write_stage_rec(std::vector<uint8_t> &b, uint32_t id, uint32_t flag, const char *s, uint32_t len) {
    wire_writer W(b);
    W.put1(id); W.put1(flag); W.put1(len);
    W.put(s, len);
}
inline void write_stage_failure(std::vector<uint8_t> &b) { write_stage_rec(b, 0xFFFFFFFFu, 0xFFFFFFFFu, nullptr, 0); }

// does the piece open with the failure record?
inline bool is_stage_failure(const uint8_t *p, size_t n) {
    wire_reader R(p, n);
    uint32_t id = 0, flag = 0, len = 0;
    return R.read(id) && R.read(flag) && R.read(len) && id == 0xFFFFFFFFu && flag == 0xFFFFFFFFu;
}

// the next record of the piece: false at its end (R.done()) or at a malformed record (!R.ok())
inline bool next_stage_rec(wire_reader &R, uint32_t n_packs, uint32_t n_clusters, stage_rec &rec) {
    if (!R.ok() || R.remaining() == 0) return false;
    if (!R.read(rec.id) || !R.read(rec.flag) || !R.read(rec.len)) return false;
    if (rec.id >= (rec.kind() == 0 ? n_packs : n_clusters)) return R.fail(rec.kind() == 0 ? "a record's pack index is out of range" : "a record's cluster index is out of range");
    rec.s = R.take<char>(rec.len);
    return R.ok();
}

// ---- 3. the cluster sets of `cluster_subsets`: the results of the subsets a rank owns ---------------------------------------------------
// Per subset [u32 subset][u32 n_clusters][u32 n_members][u64 counters[8]][i32 main_id[nc]][u32 offsets[nc + 1]][i32 member_id[nm]]
// [u8 main_rev[nc]][u8 member_rev[nm]] and zeros up to a multiple of 4; ids count within the subset.  The counters stand at 12 bytes
// past a multiple of 4, so they are copied out.  A rank that has failed sends the four bytes 0xFFFFFFFF instead.
struct cluster_set_view {
    uint32_t subset = 0, n_clusters = 0, n_members = 0;
    uint64_t counters[8] = {};
    const int32_t *main_id = nullptr, *member_id = nullptr;
    const uint32_t *offsets = nullptr;
    const uint8_t *main_rev = nullptr, *member_rev = nullptr;
};

inline void write_cluster_set(std::vector<uint8_t> &b, uint32_t subset, const rattle_cluster_set &S) {
    wire_writer W(b);
    const uint32_t nc = S.n_clusters, nm = S.offsets[nc];
    W.put1(subset); W.put1(nc); W.put1(nm);
    W.put(S.counters, 8);
    W.put(S.main_id, nc); W.put(S.offsets, (size_t)nc + 1); W.put(S.member_id, nm);
    W.put(S.main_rev, nc); W.put(S.member_rev, nm);
    W.zeros((4 - (nc + nm) % 4) % 4);
}
inline void write_cluster_sets_failure(std::vector<uint8_t> &b) { wire_writer(b).put1(0xFFFFFFFFu); }

inline bool is_cluster_sets_failure(const uint8_t *p, size_t n) {
    wire_reader R(p, n);
    uint32_t v = 0;
    return n == 4 && R.read(v) && v == 0xFFFFFFFFu;
}

// The whole piece of rank `rank`: the sets of exactly the subsets i with owner[i] == rank, each once, in any order.  seen[i] is set
// for every subset taken (the caller's, n_subsets entries: what other pieces brought stays set).
inline bool parse_cluster_sets(wire_reader &R, uint32_t n_subsets, const uint64_t *sub_off, const uint32_t *owner, uint32_t rank,
                               std::vector<uint8_t> &seen, std::vector<cluster_set_view> &out) {
    size_t expected = 0;
    for (uint32_t i = 0; i < n_subsets; ++i) expected += owner[i] == rank;
    const size_t before = out.size();
    while (R.ok() && R.remaining()) {
        cluster_set_view V;
        if (!R.read(V.subset) || !R.read(V.n_clusters) || !R.read(V.n_members)) return false;
        if (V.subset >= n_subsets) return R.fail("a subset index is out of range");
        if (owner[V.subset] != rank) return R.fail("a subset that belongs to another rank");
        if (seen[V.subset]) return R.fail("a subset arrives twice");
        const uint64_t size = sub_off[V.subset + 1] - sub_off[V.subset];
        if (V.n_members != size) return R.fail("a set's member count is not its subset's size");
        for (uint64_t &c : V.counters) R.read(c);
        V.main_id = R.take<int32_t>(V.n_clusters); V.offsets = R.take<uint32_t>((uint64_t)V.n_clusters + 1); V.member_id = R.take<int32_t>(V.n_members);
        V.main_rev = R.take<uint8_t>(V.n_clusters); V.member_rev = R.take<uint8_t>(V.n_members);
        R.skip((4 - ((uint64_t)V.n_clusters + V.n_members) % 4) % 4);
        if (!R.ok()) return false;
        if (V.offsets[0] != 0) return R.fail("a set's offsets do not start at 0");
        for (uint32_t c = 0; c < V.n_clusters; ++c) if (V.offsets[c + 1] < V.offsets[c]) return R.fail("a set's offsets decrease");
        if (V.offsets[V.n_clusters] != V.n_members) return R.fail("a set's offsets do not end at its member count");
        for (uint32_t c = 0; c < V.n_clusters; ++c) if ((uint32_t)V.main_id[c] >= size) return R.fail("a cluster's main read is not in its subset");
        for (uint32_t m = 0; m < V.n_members; ++m) if ((uint32_t)V.member_id[m] >= size) return R.fail("a member is not in its subset");
        seen[V.subset] = 1;
        out.push_back(V);
    }
    if (!R.ok()) return false;
    return out.size() - before == expected || R.fail("a subset of the rank is missing");
}

// ---- 4. the hit list of a sharded evaluation --------------------------------------------------------------------------------------------
// [u64 deltas[3]] of the request's three work counters, then the accepted pairs as [u32 seed][u32 candidate position][u32 strand]
// triples to the end of the piece (no count): indices into the request's seeds and candidates.
struct wire_hit { uint32_t seed, cand, rev; };
struct hit_list_view {
    const uint64_t *deltas = nullptr;    // [3]
    const wire_hit *hits = nullptr;
    size_t n = 0;
};

inline void write_hit_list(std::vector<uint8_t> &b, const uint64_t *deltas, const wire_hit *hits, size_t n) {
    wire_writer W(b);
    W.reserve(24 + n * sizeof(wire_hit));
    W.put(deltas, 3);
    W.put(hits, n);
}

inline bool parse_hit_list(wire_reader &R, size_t n_seeds, size_t n_cands, hit_list_view &V) {
    V.deltas = R.take<uint64_t>(3);
    if (!R.ok()) return false;
    if (R.remaining() % sizeof(wire_hit)) return R.fail("the piece ends inside a hit");
    V.n = R.remaining() / sizeof(wire_hit);
    V.hits = R.take<wire_hit>(V.n);
    if (!R.ok()) return false;
    for (size_t i = 0; i < V.n; ++i) {
        if (V.hits[i].seed >= n_seeds) return R.fail("a hit's seed is not in the request");
        if (V.hits[i].cand >= n_cands) return R.fail("a hit's candidate is not in the request");
        if (V.hits[i].rev > 1) return R.fail("a hit's strand is neither 0 nor 1");
    }
    return true;
}

}  // namespace rattle
