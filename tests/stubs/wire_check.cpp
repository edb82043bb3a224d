// The four payloads of the rank exchange (rattle_amd/csrc/wire.h) written, read back and damaged, on the host alone and meant to be
// built with -fsanitize=address,undefined (tests/test_wire.py): every piece a parser sees lies in a heap block of exactly its size,
// so a read beyond it is a sanitizer report, and a damaged piece must come back as a clean `false` with a reason.
//
// Damage, per format: every strict prefix; each count field set to 0xFFFFFFFF and to 2^63 (2^31 where the field has 32 bits); an
// offsets entry below its predecessor; a last offset beyond the piece; an id equal to its bound; the piece at an odd address.
#include "../../rattle_amd/csrc/wire.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>

using namespace rattle;
typedef std::vector<uint8_t> bytes;

static int failures = 0;
#define CHECK(cond, ...)                                                                          \
    do {                                                                                          \
        if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    } while (0)

// the piece in a heap block of its own size (shift 1: of one byte more, the piece behind the first byte)
struct placed {
    std::unique_ptr<uint8_t[]> mem;
    const uint8_t *p;
    size_t n;
    placed(const bytes &b, size_t len, int shift = 0) : mem(new uint8_t[len + shift]), p(mem.get() + shift), n(len) {
        if (len) memcpy(mem.get() + shift, b.data(), len);
    }
};

template <typename T>
static void poke(bytes &b, size_t at, T v) { memcpy(b.data() + at, &v, sizeof(T)); }
template <typename T>
static T peek(const bytes &b, size_t at) { T v; memcpy(&v, b.data() + at, sizeof(T)); return v; }

// a parser under test: true if it accepts the piece
typedef std::function<bool(const uint8_t *, size_t, std::string &)> accept_fn;

static void expect_rejected(const char *what, const accept_fn &accept, const bytes &b, size_t len, int shift = 0) {
    placed P(b, len, shift);
    std::string why;
    const bool ok = accept(P.p, P.n, why);
    CHECK(!ok, "%s: accepted (length %zu of %zu, shift %d)", what, len, b.size(), shift);
    CHECK(ok || (!why.empty() && why != "no error"), "%s: rejected without a reason", what);
}
template <typename T>
static void expect_rejected_with(const char *what, const accept_fn &accept, bytes b, size_t at, T v) {
    poke(b, at, v);
    expect_rejected(what, accept, b, b.size());
}
// count field of 64 / 32 bits at `at`
static void damage_count64(const char *what, const accept_fn &accept, const bytes &b, size_t at) {
    expect_rejected_with<uint64_t>(what, accept, b, at, 0xFFFFFFFFull);
    expect_rejected_with<uint64_t>(what, accept, b, at, 1ull << 63);
    expect_rejected_with<uint64_t>(what, accept, b, at, ~0ull);
}
static void damage_count32(const char *what, const accept_fn &accept, const bytes &b, size_t at) {
    expect_rejected_with<uint32_t>(what, accept, b, at, 0xFFFFFFFFu);
    expect_rejected_with<uint32_t>(what, accept, b, at, 1u << 31);
}

// ---- 1. the gather piece ---------------------------------------------------------------------------------------------------------------
struct read_set_data {
    std::vector<int32_t> read_id, cluster_id, n_reads;
    std::vector<uint32_t> pack;
    std::vector<uint64_t> off;
    std::string seq, qual;
    rattle_read_set S;
    read_set_data(const std::vector<uint32_t> &lens, int salt) {
        off.push_back(0);
        for (size_t i = 0; i < lens.size(); ++i) {
            read_id.push_back((int32_t)(100 * salt + i)); cluster_id.push_back((int32_t)(salt + 2 * i)); n_reads.push_back((int32_t)(i % 2));
            pack.push_back(i == 0 ? 0xFFFFFFFFu : (uint32_t)(7 * i + salt));
            for (uint32_t k = 0; k < lens[i]; ++k) { seq.push_back("ACGT"[(k + i + salt) % 4]); qual.push_back((char)('!' + (k * 3 + i) % 40)); }
            off.push_back(seq.size());
        }
        // (the arrays of an empty set are still addresses, as the library's are)
        read_id.push_back(0); cluster_id.push_back(0); n_reads.push_back(0); pack.push_back(0);
        S.n = (uint32_t)lens.size();
        S.read_id = read_id.data(); S.cluster_id = cluster_id.data(); S.n_reads = n_reads.data(); S.off = off.data();
        S.seq = &seq[0]; S.qual = &qual[0];
    }
};

struct gather_case {
    read_set_data cor, unc;
    std::vector<int32_t> k_cid, k_rid;
    std::vector<uint32_t> k_pack, k_stage;
    std::vector<uint64_t> k_off;
    std::vector<std::vector<uint32_t>> rep;
    std::vector<uint32_t *> rep_p;
    bool has_rep;
    rattle_correction L;
    gather_case(const std::vector<uint32_t> &cor_lens, const std::vector<uint32_t> &unc_lens, const std::vector<uint32_t> &skip_reads, bool report)
        : cor(cor_lens, 1), unc(unc_lens, 2), has_rep(report) {
        k_off.push_back(0);
        for (size_t i = 0; i < skip_reads.size(); ++i) {
            k_cid.push_back((int32_t)(3 + i)); k_pack.push_back((uint32_t)i); k_stage.push_back((uint32_t)(1 + i % 3));
            for (uint32_t k = 0; k < skip_reads[i]; ++k) k_rid.push_back((int32_t)(50 + 10 * i + k));
            k_off.push_back(k_rid.size());
        }
        k_cid.push_back(0); k_pack.push_back(0); k_stage.push_back(0); k_rid.push_back(0);
        memset(&L, 0, sizeof(L));
        L.corrected = cor.S; L.uncorrected = unc.S;
        L.corrected_pack = cor.pack.data(); L.uncorrected_pack = unc.pack.data();
        L.skipped.n = (uint32_t)skip_reads.size();
        L.skipped.cluster_id = k_cid.data(); L.skipped.pack = k_pack.data(); L.skipped.stage = k_stage.data();
        L.skipped.read_off = k_off.data(); L.skipped.read_id = k_rid.data();
        for (int i = 0; i < 8; ++i) L.counters[i] = 1000 + 17 * i;
        for (int f = 0; f < WIRE_REP_FIELDS; ++f) {
            rep.emplace_back();
            for (uint32_t i = 0; i < cor.S.n; ++i) rep.back().push_back(1000 * f + i);
            rep.back().push_back(0);
        }
        for (auto &v : rep) rep_p.push_back(v.data());
    }
    bytes piece() const { bytes b; write_gather_piece(b, L, has_rep ? rep_p.data() : nullptr); return b; }
};

static bool same_set(const piece_view &V, const read_set_data &D) {
    const uint32_t n = D.S.n;
    if (V.n != n) return false;
    if (memcmp(V.off, D.off.data(), (n + 1) * 8)) return false;
    if (n && (memcmp(V.read_id, D.read_id.data(), n * 4) || memcmp(V.cluster_id, D.cluster_id.data(), n * 4) || memcmp(V.n_reads, D.n_reads.data(), n * 4) ||
              memcmp(V.pack, D.pack.data(), n * 4))) return false;
    const size_t tot = D.seq.size();
    return tot == 0 || (memcmp(V.seq, D.seq.data(), tot) == 0 && memcmp(V.qual, D.qual.data(), tot) == 0);
}

static void check_gather(const char *name, const gather_case &G) {
    const bytes b = G.piece();
    CHECK(b.size() % 8 == 0, "%s: the piece is %zu bytes, no multiple of 8", name, b.size());
    {
        placed P(b, b.size());
        wire_reader R(P.p, P.n);
        gather_view V;
        const bool ok = parse_gather_piece(R, V);
        CHECK(ok, "%s: the intact piece is rejected: %s", name, R.reason());
        if (ok) {
            CHECK(same_set(V.corrected, G.cor) && same_set(V.uncorrected, G.unc), "%s: a read set differs", name);
            const uint64_t n = G.L.skipped.n, tot = G.k_off[n];
            CHECK(V.skipped.n == n && memcmp(V.skipped.read_off, G.k_off.data(), (n + 1) * 8) == 0, "%s: the skip list's offsets differ", name);
            CHECK(!n || (memcmp(V.skipped.cluster_id, G.k_cid.data(), n * 4) == 0 && memcmp(V.skipped.pack, G.k_pack.data(), n * 4) == 0 &&
                         memcmp(V.skipped.stage, G.k_stage.data(), n * 4) == 0), "%s: the skip list differs", name);
            CHECK(!tot || memcmp(V.skipped.read_id, G.k_rid.data(), tot * 4) == 0, "%s: the skip list's reads differ", name);
            CHECK(memcmp(V.counters, G.L.counters, 64) == 0, "%s: the counters differ", name);
            CHECK(V.corrected.has_rep == G.has_rep && !V.uncorrected.has_rep, "%s: the report flag differs", name);
            if (G.has_rep) for (int f = 0; f < WIRE_REP_FIELDS; ++f)
                CHECK(G.cor.S.n == 0 || memcmp(V.corrected.rep[f], G.rep[f].data(), G.cor.S.n * 4) == 0, "%s: report field %d differs", name, f);
        }
    }
    const accept_fn accept = [](const uint8_t *p, size_t n, std::string &why) {
        wire_reader R(p, n);
        gather_view V;
        const bool ok = parse_gather_piece(R, V);
        why = R.reason();
        return ok;
    };
    for (size_t len = 0; len < b.size(); ++len) expect_rejected(name, accept, b, len);      // exact consumption: no strict prefix passes
    expect_rejected(name, accept, b, b.size(), 1);
    {
        bytes longer = b;
        longer.resize(b.size() + 8, 0);
        expect_rejected(name, accept, longer, longer.size());
    }
    // where the parts start: the two sets, then the skip list, then (behind its arrays and the eight counters) the flag
    bytes s1, s2;
    write_read_set(s1, G.L.corrected, G.L.corrected_pack); write_read_set(s2, G.L.uncorrected, G.L.uncorrected_pack);
    const size_t at_set[2] = {0, s1.size()}, at_skip = s1.size() + s2.size();
    const uint64_t kn = G.L.skipped.n, ktot = G.k_off[kn];
    const size_t at_flag = at_skip + 8 + (kn + 1) * 8 + 12 * kn + 4 * ktot + (((3 * kn + ktot) & 1) ? 4 : 0) + 64;
    CHECK(at_flag + 8 + (G.has_rep ? 40 * (size_t)G.cor.S.n : 0) == b.size(), "%s: the test's own layout is off", name);
    for (int s = 0; s < 2; ++s) {
        const read_set_data &D = s ? G.unc : G.cor;
        const uint64_t n = D.S.n;
        damage_count64(name, accept, b, at_set[s]);
        const size_t at_off = at_set[s] + 8;
        expect_rejected_with<uint64_t>(name, accept, b, at_off, 1);                                   // off[0] != 0
        expect_rejected_with<uint64_t>(name, accept, b, at_off + 8 * n, b.size());                    // off[n] beyond the piece
        expect_rejected_with<uint64_t>(name, accept, b, at_off + 8 * n, 1ull << 63);
        expect_rejected_with<uint64_t>(name, accept, b, at_off + 8 * n, ~0ull);
        for (uint64_t i = 1; i <= n; ++i) if (D.off[i - 1] > 0) expect_rejected_with<uint64_t>(name, accept, b, at_off + 8 * i, D.off[i - 1] - 1);
    }
    damage_count64(name, accept, b, at_skip);
    expect_rejected_with<uint64_t>(name, accept, b, at_skip + 8, 1);
    expect_rejected_with<uint64_t>(name, accept, b, at_skip + 8 + 8 * kn, b.size());
    expect_rejected_with<uint64_t>(name, accept, b, at_skip + 8 + 8 * kn, 1ull << 63);
    for (uint64_t i = 1; i <= kn; ++i) if (G.k_off[i - 1] > 0) expect_rejected_with<uint64_t>(name, accept, b, at_skip + 8 + 8 * i, G.k_off[i - 1] - 1);
    damage_count64(name, accept, b, at_flag);
    expect_rejected_with<uint64_t>(name, accept, b, at_flag, 2);
    if (G.cor.S.n) expect_rejected_with<uint64_t>(name, accept, b, at_flag, G.has_rep ? 0 : 1);       // the arrays must match the flag
}

// ---- 2. stage records ------------------------------------------------------------------------------------------------------------------
static void check_stage() {
    const uint32_t n_packs = 4, n_clusters = 3;
    struct rec { uint32_t id, flag; std::string s; };
    const std::vector<rec> recs = {{1, 0u, "ACG"}, {0, 1u, ""}, {3, 2u << 1, ""}, {2, 1u, "ACGTA"}, {0, 0u, "T"}, {1, 1u | (3u << 1), ""}};
    bytes b;
    std::vector<size_t> ends{0};
    for (const rec &r : recs) { write_stage_rec(b, r.id, r.flag, r.s.empty() ? nullptr : r.s.data(), (uint32_t)r.s.size()); ends.push_back(b.size()); }
    // k records if the piece parses, -1 if it is rejected; what was read is compared with the records written
    auto parse = [&](const uint8_t *p, size_t n, std::string &why) {
        wire_reader R(p, n);
        stage_rec v;
        int k = 0;
        while (next_stage_rec(R, n_packs, n_clusters, v)) {
            const rec &w = recs[(size_t)k];
            CHECK(v.id == w.id && v.flag == w.flag && v.len == w.s.size() && (v.len == 0 || memcmp(v.s, w.s.data(), v.len) == 0), "stage record %d differs", k);
            CHECK(v.kind() == (w.flag & 1u) && v.dead() == w.flag >> 1, "stage record %d: kind / dead", k);
            ++k;
        }
        why = R.reason();
        CHECK(R.ok() == R.done(), "a stage piece that ends well is consumed");
        return R.ok() ? k : -1;
    };
    for (int shift = 0; shift < 2; ++shift)                    // no array in this format: any address will do
        for (size_t len = 0; len <= b.size(); ++len) {
            placed P(b, len, shift);
            std::string why;
            const int k = parse(P.p, P.n, why);
            int want = -1;
            for (size_t i = 0; i < ends.size(); ++i) if (ends[i] == len) want = (int)i;
            CHECK(k == want, "stage prefix of %zu bytes: %d records, expected %d (%s)", len, k, want, why.c_str());
        }
    const accept_fn accept = [&](const uint8_t *p, size_t n, std::string &why) {
        wire_reader R(p, n);
        stage_rec v;
        while (next_stage_rec(R, n_packs, n_clusters, v)) {}
        why = R.reason();
        return R.ok();
    };
    for (size_t i = 0; i < recs.size(); ++i) {
        // the length: as it stands it reaches beyond the piece for every record but a last one without bytes
        damage_count32("stage len", accept, b, ends[i] + 8);
        expect_rejected_with<uint32_t>("stage len", accept, b, ends[i] + 8, (uint32_t)(b.size() - ends[i] - 12 + 1));
        expect_rejected_with<uint32_t>("stage id", accept, b, ends[i], (recs[i].flag & 1u) ? n_clusters : n_packs);      // an id equal to its bound
        expect_rejected_with<uint32_t>("stage id", accept, b, ends[i], 0xFFFFFFFFu);
    }
    // the failure record
    bytes f;
    write_stage_failure(f);
    CHECK(f.size() == 12 && peek<uint32_t>(f, 0) == 0xFFFFFFFFu && peek<uint32_t>(f, 4) == 0xFFFFFFFFu && peek<uint32_t>(f, 8) == 0, "the failure record's bytes");
    for (size_t len = 0; len <= f.size(); ++len) {
        placed P(f, len);
        CHECK(is_stage_failure(P.p, P.n) == (len == 12), "failure record, %zu bytes", len);
    }
    { placed P(b, b.size()); CHECK(!is_stage_failure(P.p, P.n), "a piece of records is no failure record"); }
    expect_rejected("stage failure record as a record", accept, f, f.size());
}

// ---- 3. cluster sets -------------------------------------------------------------------------------------------------------------------
struct cluster_set_data {
    std::vector<int32_t> main_id, member_id;
    std::vector<uint8_t> main_rev, member_rev;
    std::vector<uint32_t> offsets;
    rattle_cluster_set S;
    // nc clusters over the `size` reads of a subset, dealt out in turn
    cluster_set_data(uint32_t nc, uint32_t size, int salt) {
        std::vector<std::vector<int32_t>> mem(nc);
        for (uint32_t i = 0; i < size; ++i) mem[i % nc].push_back((int32_t)((i + salt) % size));
        offsets.push_back(0);
        for (uint32_t c = 0; c < nc; ++c) {
            main_id.push_back(mem[c].empty() ? 0 : mem[c][0]); main_rev.push_back((uint8_t)(c & 1));
            for (int32_t m : mem[c]) { member_id.push_back(m); member_rev.push_back((uint8_t)((m + salt) & 1)); }
            offsets.push_back((uint32_t)member_id.size());
        }
        main_id.push_back(0); member_id.push_back(0); main_rev.push_back(0); member_rev.push_back(0);
        memset(&S, 0, sizeof(S));
        S.n_clusters = nc;
        S.main_id = main_id.data(); S.main_rev = main_rev.data(); S.offsets = offsets.data(); S.member_id = member_id.data(); S.member_rev = member_rev.data();
        for (int i = 0; i < 8; ++i) S.counters[i] = ((uint64_t)salt << 40) + 11 * i;
    }
};

static void check_cluster_sets() {
    // the subsets of rank 1, with (n_clusters + size) % 4 = 0, 0, 1, 2, 3, and one of rank 0 between them
    const uint32_t n_subsets = 6, rank = 1;
    const uint32_t size[6] = {0, 3, 4, 2, 4, 5}, ncl[6] = {0, 1, 1, 1, 2, 2}, owner[6] = {1, 1, 1, 0, 1, 1};
    uint64_t sub_off[7] = {0};
    for (uint32_t i = 0; i < n_subsets; ++i) sub_off[i + 1] = sub_off[i] + size[i];
    std::vector<cluster_set_data> D;
    for (uint32_t i = 0; i < n_subsets; ++i) D.emplace_back(ncl[i], size[i], (int)i + 1);
    const uint32_t order[5] = {5, 4, 2, 1, 0};               // largest first, as the ranks send them
    bytes b;
    std::vector<size_t> at;                                   // where each record starts
    for (uint32_t i : order) {
        at.push_back(b.size());
        write_cluster_set(b, i, D[i].S);
        CHECK(b.size() % 4 == 0, "a cluster set record is padded to 4 bytes");
        CHECK((b.size() - at.back()) == 76 + 4 * (size_t)ncl[i] + 4 * ((size_t)ncl[i] + 1) + 4 * (size_t)size[i] + (ncl[i] + size[i] + 3) / 4 * 4, "cluster set record size");
    }
    at.push_back(b.size());
    auto parse = [&](const uint8_t *p, size_t n, std::string &why, std::vector<cluster_set_view> &out) {
        wire_reader R(p, n);
        std::vector<uint8_t> seen(n_subsets, 0);
        const bool ok = parse_cluster_sets(R, n_subsets, sub_off, owner, rank, seen, out);
        why = R.reason();
        if (ok) for (uint32_t i = 0; i < n_subsets; ++i) CHECK(seen[i] == (owner[i] == rank), "seen[%u] after an accepted piece", i);
        return ok;
    };
    {
        placed P(b, b.size());
        std::string why;
        std::vector<cluster_set_view> V;
        const bool ok = parse(P.p, P.n, why, V);
        CHECK(ok && V.size() == 5, "the intact cluster sets are rejected: %s", why.c_str());
        for (size_t k = 0; ok && k < V.size(); ++k) {
            const cluster_set_data &W = D[order[k]];
            const uint32_t nc = ncl[order[k]], nm = size[order[k]];
            CHECK(V[k].subset == order[k] && V[k].n_clusters == nc && V[k].n_members == nm, "cluster set %zu: header", k);
            CHECK(memcmp(V[k].counters, W.S.counters, 64) == 0, "cluster set %zu: counters", k);
            CHECK(memcmp(V[k].offsets, W.offsets.data(), (nc + 1) * 4) == 0, "cluster set %zu: offsets", k);
            CHECK(!nc || (memcmp(V[k].main_id, W.main_id.data(), nc * 4) == 0 && memcmp(V[k].main_rev, W.main_rev.data(), nc) == 0), "cluster set %zu: mains", k);
            CHECK(!nm || (memcmp(V[k].member_id, W.member_id.data(), nm * 4) == 0 && memcmp(V[k].member_rev, W.member_rev.data(), nm) == 0), "cluster set %zu: members", k);
        }
    }
    const accept_fn accept = [&](const uint8_t *p, size_t n, std::string &why) { std::vector<cluster_set_view> V; return parse(p, n, why, V); };
    for (size_t len = 0; len < b.size(); ++len) expect_rejected("cluster sets", accept, b, len);      // completeness: a prefix of whole records lacks a subset
    expect_rejected("cluster sets", accept, b, b.size(), 1);
    for (size_t k = 0; k + 1 < at.size(); ++k) {
        const uint32_t i = order[k], nc = ncl[i], nm = size[i];
        {   // the record removed whole: its subset never arrives
            bytes cut(b.begin(), b.begin() + at[k]);
            cut.insert(cut.end(), b.begin() + at[k + 1], b.end());
            expect_rejected("cluster sets, one removed", accept, cut, cut.size());
        }
        expect_rejected_with<uint32_t>("cluster sets: subset of another rank", accept, b, at[k], 3);
        expect_rejected_with<uint32_t>("cluster sets: subset == n_subsets", accept, b, at[k], n_subsets);
        expect_rejected_with<uint32_t>("cluster sets: subset twice", accept, b, at[k], order[(k + 1) % 5]);
        damage_count32("cluster sets: n_clusters", accept, b, at[k] + 4);
        expect_rejected_with<uint32_t>("cluster sets: n_clusters", accept, b, at[k] + 4, nc + 1);
        damage_count32("cluster sets: n_members", accept, b, at[k] + 8);
        expect_rejected_with<uint32_t>("cluster sets: n_members", accept, b, at[k] + 8, nm + 1);
        const size_t at_main = at[k] + 76, at_off = at_main + 4 * (size_t)nc, at_mem = at_off + 4 * ((size_t)nc + 1);
        expect_rejected_with<uint32_t>("cluster sets: offsets[0]", accept, b, at_off, 1);
        expect_rejected_with<uint32_t>("cluster sets: offsets[nc]", accept, b, at_off + 4 * (size_t)nc, nm + 1);
        expect_rejected_with<uint32_t>("cluster sets: offsets[nc]", accept, b, at_off + 4 * (size_t)nc, 0xFFFFFFFFu);
        for (uint32_t c = 1; c <= nc; ++c) if (D[i].offsets[c - 1] > 0) expect_rejected_with<uint32_t>("cluster sets: offsets decrease", accept, b, at_off + 4 * (size_t)c, D[i].offsets[c - 1] - 1);
        for (uint32_t c = 0; c < nc; ++c) {
            expect_rejected_with<uint32_t>("cluster sets: main id", accept, b, at_main + 4 * (size_t)c, nm);
            expect_rejected_with<int32_t>("cluster sets: main id", accept, b, at_main + 4 * (size_t)c, -1);
        }
        for (uint32_t m = 0; m < nm; ++m) expect_rejected_with<uint32_t>("cluster sets: member id", accept, b, at_mem + 4 * (size_t)m, nm);
    }
    // a rank without subsets sends nothing, and nothing is all it may send
    {
        const uint32_t all0[6] = {0, 0, 0, 0, 0, 0};
        placed P(b, 0);
        wire_reader R(P.p, 0);
        std::vector<uint8_t> seen(n_subsets, 0);
        std::vector<cluster_set_view> V;
        CHECK(parse_cluster_sets(R, n_subsets, sub_off, all0, rank, seen, V) && V.empty(), "the empty piece of a rank without subsets");
    }
    bytes f;
    write_cluster_sets_failure(f);
    CHECK(f.size() == 4 && peek<uint32_t>(f, 0) == 0xFFFFFFFFu, "the failure marker's bytes");
    for (size_t len = 0; len <= f.size(); ++len) { placed P(f, len); CHECK(is_cluster_sets_failure(P.p, P.n) == (len == 4), "failure marker, %zu bytes", len); }
    { placed P(b, b.size()); CHECK(!is_cluster_sets_failure(P.p, P.n), "a piece of sets is no failure marker"); }
    expect_rejected("cluster sets: the failure marker as a record", accept, f, f.size());
}

// ---- 4. hit lists ----------------------------------------------------------------------------------------------------------------------
static void check_hit_lists() {
    const size_t n_seeds = 3, n_cands = 4;
    const uint64_t deltas[3] = {12, 5, 1ull << 40};
    const wire_hit hits[2] = {{2, 3, 1}, {0, 0, 0}};
    for (size_t nh : {(size_t)0, (size_t)2}) {
        bytes b;
        write_hit_list(b, deltas, hits, nh);
        CHECK(b.size() == 24 + 12 * nh, "hit list size");
        for (size_t len = 0; len <= b.size(); ++len) {
            placed P(b, len);
            wire_reader R(P.p, P.n);
            hit_list_view V;
            const bool ok = parse_hit_list(R, n_seeds, n_cands, V);
            const bool boundary = len >= 24 && (len - 24) % 12 == 0;
            CHECK(ok == boundary, "hit list prefix of %zu bytes: %s", len, R.reason());
            if (ok) {
                CHECK(V.n == (len - 24) / 12 && R.done() && memcmp(V.deltas, deltas, 24) == 0, "hit list prefix of %zu bytes: the counters or the count", len);
                CHECK(V.n == 0 || memcmp(V.hits, hits, V.n * 12) == 0, "hit list prefix of %zu bytes: the hits", len);
            }
        }
        const accept_fn accept = [&](const uint8_t *p, size_t n, std::string &why) {
            wire_reader R(p, n);
            hit_list_view V;
            const bool ok = parse_hit_list(R, n_seeds, n_cands, V);
            why = R.reason();
            return ok;
        };
        expect_rejected("hit list at an odd address", accept, b, b.size(), 1);
        for (size_t i = 0; i < nh; ++i) {
            expect_rejected_with<uint32_t>("hit list: seed", accept, b, 24 + 12 * i, (uint32_t)n_seeds);
            expect_rejected_with<uint32_t>("hit list: seed", accept, b, 24 + 12 * i, 0xFFFFFFFFu);
            expect_rejected_with<uint32_t>("hit list: candidate", accept, b, 24 + 12 * i + 4, (uint32_t)n_cands);
            expect_rejected_with<uint32_t>("hit list: candidate", accept, b, 24 + 12 * i + 4, 1u << 31);
            expect_rejected_with<uint32_t>("hit list: strand", accept, b, 24 + 12 * i + 8, 2);
        }
    }
}

// ---- the reader itself -----------------------------------------------------------------------------------------------------------------
static void check_reader() {
    bytes b(24);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)i;
    placed P(b, b.size());
    wire_reader R(P.p, P.n);
    uint32_t v = 0;
    CHECK(R.read(v) && v == 0x03020100u && R.remaining() == 20, "scalar read");
    CHECK(R.take<uint64_t>(1) == nullptr && !R.ok(), "an 8-byte array at offset 4 is misaligned");
    const std::string first = R.reason();
    CHECK(!R.read(v) && !R.skip(0) && R.take<uint8_t>(1) == nullptr && first == R.reason() && !R.done(), "a failed read is sticky and keeps its reason");
    wire_reader Q(P.p, P.n);
    CHECK(Q.take<uint64_t>((1ull << 61) + 1) == nullptr && !Q.ok(), "a count whose byte size overflows");
    wire_reader S(P.p, P.n);
    CHECK(S.take<uint64_t>(2) == (const uint64_t *)P.p && S.skip(4) && S.take<uint32_t>(1) != nullptr && S.done(), "views and skip up to the end");
    CHECK(!S.skip(1) && !S.ok(), "skip beyond the end");
}

int main() {
    check_reader();
    // read sets of 0, 1 and 3 records; 2 * bases % 8 zero (4 bases) and non-zero (5, 1); skip list with 3 n + reads odd (1, 2), even (2, 2) and
    // empty; report present, absent, and present for no record
    check_gather("gather A", gather_case({1, 2, 2}, {}, {2}, true));
    check_gather("gather B", gather_case({4}, {0, 3, 1}, {0, 2}, false));
    check_gather("gather C", gather_case({}, {5}, {}, true));
    check_gather("gather D", gather_case({3, 0, 2}, {1}, {1, 0, 3}, false));
    check_stage();
    check_cluster_sets();
    check_hit_lists();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("WIRE_CHECK_OK\n");
    return 0;
}
