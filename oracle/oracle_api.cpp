// ORACLE (test infrastructure, never shipped in the product path).
// extern "C" surface over the restatement for ctypes (tests/, smoke(), bench cpu_baseline).
#include <chrono>
#include <cstring>

#include "orc_cluster.hpp"
#include "orc_correct.hpp"
#include "orc_io.hpp"
#include "orc_poa.hpp"

using namespace orc;

static read_set_t make_reads(const char *seqs, const uint64_t *off, uint32_t n, const char *quals) {
    read_set_t rs(n);
    for (uint32_t i = 0; i < n; ++i) {
        rs[i].seq.assign(seqs + off[i], seqs + off[i + 1]);
        rs[i].ann = std::to_string(i);
        rs[i].header = "@r" + std::to_string(i);
        if (quals) rs[i].quality.assign(quals + off[i], quals + off[i + 1]);
    }
    return rs;
}

extern "C" {

// k-mer lists + bit-vectors of one read.  Lists hold max(L-k,0) entries.
void orc_extract_kmers(const char *seq, uint32_t len, int k, int both, uint32_t *fwd_hash, int32_t *fwd_pos,
                       uint32_t *rev_hash, int32_t *rev_pos, uint64_t *bv_fwd, uint64_t *bv_rev) {
    read_kmers_t r = extract_kmers_from_read(std::string(seq, len), k, both != 0);
    for (size_t i = 0; i < r.list_forward.size(); ++i) {
        fwd_hash[i] = r.list_forward[i].first; fwd_pos[i] = r.list_forward[i].second;
        if (both) { rev_hash[i] = r.list_reverse[i].first; rev_pos[i] = r.list_reverse[i].second; }
    }
    for (int w = 0; w < 64; ++w) {
        uint64_t a = 0, b = 0;
        for (int t = 0; t < 64; ++t) {
            if (r.bv_forward[w * 64 + t]) a |= 1ull << t;
            if (r.bv_reverse[w * 64 + t]) b |= 1ull << t;
        }
        bv_fwd[w] = a; bv_rev[w] = b;
    }
}

// Full pair comparison (get_common_kmers + calc_similarity + var) of read a vs read b
// (b's forward strand if strand==0, else b's reverse-complement strand).
void orc_pair_score(const char *a, uint32_t la, const char *b, uint32_t lb, int k, int strand, int32_t *bases,
                    int32_t *hc_bases, int32_t *n_dist, double *variance, int32_t *n_matches, int32_t *dist_out,
                    int32_t dist_cap) {
    read_kmers_t ka = extract_kmers_from_read(std::string(a, la), k, false);
    read_kmers_t kb = extract_kmers_from_read(std::string(b, lb), k, true);
    auto common = get_common_kmers(ka.list_forward, strand ? kb.list_reverse : kb.list_forward);
    auto sim = calc_similarity(common, k);
    *bases = sim.bases; *hc_bases = sim.hc_bases; *n_dist = (int32_t)sim.distances.size();
    *variance = var(sim.distances);
    *n_matches = (int32_t)common.size();
    for (int i = 0; i < (int)sim.distances.size() && i < dist_cap; ++i) dist_out[i] = sim.distances[i];
}

double orc_var(const int32_t *v, uint32_t n) { return var(std::vector<int>(v, v + n)); }

// cluster_reads on reads ALREADY in processing order (length-descending).  Output:
// flattened clusters with local ids.  Returns number of clusters; member arrays must hold n.
// counters[0..2] = pair tests, full comparisons, matches.
int32_t orc_cluster_reads(const char *seqs, const uint64_t *off, uint32_t n, int k, double t_s, double t_v, double bvB,
                          double bvb, double bvf, double repr_pct, int is_rna, int32_t *cl_main_id, uint8_t *cl_main_rev,
                          uint32_t *cl_off, int32_t *mem_id, uint8_t *mem_rev, uint64_t *counters) {
    read_set_t rs = make_reads(seqs, off, n, nullptr);
    work_counters_t wc;
    cluster_set_t cs = cluster_reads(rs, k, t_s, t_v, bvB, bvb, bvf, 0, false, repr_pct, is_rna != 0, &wc);
    uint32_t p = 0;
    for (size_t c = 0; c < cs.size(); ++c) {
        cl_main_id[c] = cs[c].main_seq.seq_id; cl_main_rev[c] = cs[c].main_seq.rev; cl_off[c] = p;
        for (auto &s : cs[c].seqs) { mem_id[p] = s.seq_id; mem_rev[p] = s.rev; ++p; }
    }
    cl_off[cs.size()] = p;
    if (counters) { counters[0] = wc.pair_tests; counters[1] = wc.full_cmp; counters[2] = wc.matches; }
    return (int32_t)cs.size();
}

// POA MSA of n sequences (correct.cpp:398-405 call pattern).  Rows are written
// back-to-back into msa_out (n * width bytes); returns width, or -1 if cap too small.
int64_t orc_poa_msa(const char *seqs, const uint64_t *off, uint32_t n, char *msa_out, uint64_t cap, uint64_t *cells) {
    std::vector<std::string> v(n);
    for (uint32_t i = 0; i < n; ++i) v[i].assign(seqs + off[i], seqs + off[i + 1]);
    uint64_t c = 0;
    std::vector<std::string> msa = poa_msa(v, &c);
    if (cells) *cells = c;
    size_t W = msa.empty() ? 0 : msa[0].size();
    if (W * n > cap) return -1;
    for (uint32_t i = 0; i < n; ++i) memcpy(msa_out + (size_t)i * W, msa[i].data(), W);
    return (int64_t)W;
}

// Whole `correct` on in-memory reads (file order, with qualities) + clusters in the hps
// byte encoding.  Writes the three FASTQ texts into malloc'd buffers (caller frees with orc_free).
int32_t orc_correct(const char *seqs, const char *quals, const uint64_t *off, uint32_t n, const char *const *headers,
                    const uint8_t *clusters_hps, uint64_t clusters_len, double min_occ, double gap_occ, int split,
                    int min_reads, char **corrected, char **uncorrected, char **consensi, uint64_t *counters,
                    uint32_t n_pack_orders, const uint32_t *po_cluster, const uint32_t *po_offsets, const uint32_t *po_perm) {
    read_set_t rs = make_reads(seqs, off, n, quals);
    for (uint32_t i = 0; i < n; ++i) { rs[i].ann = "+"; if (headers) rs[i].header = headers[i]; }
    cluster_set_t cs;
    std::string b((const char *)clusters_hps, clusters_len);
    if (!hps_decode(b, 3, cs) && !hps_decode(b, 2, cs)) return -1;
    correct_counters_t cc;
    std::map<int, std::vector<int>> po;
    for (uint32_t i = 0; i < n_pack_orders; ++i) po[(int)po_cluster[i]] = std::vector<int>(po_perm + po_offsets[i], po_perm + po_offsets[i + 1]);
    correction_results_t R = correct_reads(cs, rs, min_occ, gap_occ, 30.0, split, min_reads, {}, &cc, n_pack_orders ? &po : nullptr);
    auto dump = [](const read_set_t &v) {
        std::string s;
        for (auto &r : v) s += r.header + "\n" + r.seq + "\n" + r.ann + "\n" + r.quality + "\n";
        char *p = (char *)malloc(s.size() + 1);
        memcpy(p, s.data(), s.size());
        p[s.size()] = 0;
        return p;
    };
    *corrected = dump(R.corrected); *uncorrected = dump(R.uncorrected); *consensi = dump(R.consensi);
    if (counters) { counters[0] = cc.dp_cells; counters[1] = cc.packs; counters[2] = cc.alignments; }
    return 0;
}


// fix_msa_ends (correct.cpp:32-92) on hand-built MSA rows: rows are `width` bytes each and are rewritten in place; the
// reads' sequences / qualities (concatenated at off[]) are mutated the way the reference mutates them, and their new
// lengths returned (the bytes themselves are moved to the front of each read's slot).
void orc_fix_msa_ends(char *rows, uint32_t n, uint32_t width, char *seqs, char *quals, const uint64_t *off, uint32_t *len_out) {
    read_set_t rs;
    msa_t msa;
    for (uint32_t i = 0; i < n; ++i) {
        rs.push_back(read_t{"", std::string(seqs + off[i], seqs + off[i + 1]), "+", std::string(quals + off[i], quals + off[i + 1])});
        msa.push_back(std::string(rows + (size_t)i * width, width));
    }
    fix_msa_ends(rs, msa);
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(rows + (size_t)i * width, msa[i].data(), width);
        memcpy(seqs + off[i], rs[i].seq.data(), rs[i].seq.size());
        memcpy(quals + off[i], rs[i].quality.data(), rs[i].quality.size());
        len_out[i] = (uint32_t)rs[i].seq.size();
    }
}

// The post-MSA half of one pack (correct.cpp:407-409 after POA #1, :438-445 / :533-535 after POA #2 / #3) on an explicit MSA:
// fix_msa_ends, generate_consensus_vector and, in mode 1, correct_read_pack.  rows: n rows of `width` bytes; quals: the quality
// bytes of every row's bases at qoff[] (NULL in mode 2: 'K', what the reference gives a consensus).  Out: the fixed rows, every
// row's window (first / last non-gap column, width / -1 if none) and the bases erased per phase [2n]; per column the winner, its
// occ and total_occ, the bits of its mean error and (mode 1, winner not '-') the phred_symbol of it; the corrected reads
// (mode 1; out_off [n+1], a read that came out empty is flagged) and the consensus.  The vote order is set_cv_order's.
void orc_post_msa(const char *rows, uint32_t n, uint32_t width, const char *quals, const uint64_t *qoff, double min_occ, double gap_occ,
                  double err_ratio, int mode, char *rows_out, int32_t *rfirst, int32_t *rlast, uint32_t *erased, char *winner,
                  int32_t *occ, int32_t *total_occ, uint64_t *err_bits, uint8_t *sym, char *out_seq, char *out_qual, uint64_t *out_off,
                  uint8_t *empty, char *cons, uint32_t *cons_len) {
    read_set_t rs(n);
    msa_t msa(n);
    for (uint32_t i = 0; i < n; ++i) {
        msa[i].assign(rows + (size_t)i * width, width);
        for (char c : msa[i]) if (c != '-') rs[i].seq += c;
        rs[i].header = std::to_string(i);
        rs[i].ann = "+";
        rs[i].quality = quals ? std::string(quals + qoff[i], quals + qoff[i + 1]) : std::string(rs[i].seq.size(), 'K');
    }
    std::vector<std::array<uint32_t, 2>> er;
    fix_msa_ends(rs, msa, &er);
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(rows_out + (size_t)i * width, msa[i].data(), width);
        const size_t a = msa[i].find_first_not_of('-'), b = msa[i].find_last_not_of('-');
        rfirst[i] = a == std::string::npos ? (int32_t)width : (int32_t)a;
        rlast[i] = b == std::string::npos ? -1 : (int32_t)b;
        erased[2 * i] = er[i][0]; erased[2 * i + 1] = er[i][1];
    }
    consensus_vector_t cv = generate_consensus_vector(rs, msa);
    for (size_t k = 0; k < cv.consensus_nt.size(); ++k) {
        const char w = cv.consensus_nt[k];
        const pos_info_t &pi = cv.nt_info[k][cv_slot(w)];
        winner[k] = w; occ[k] = pi.occ; total_occ[k] = pi.total_occ;
        memcpy(&err_bits[k], &pi.err, 8);
        sym[k] = mode == 1 && w != '-' ? (uint8_t)phred_symbol(pi.err) : 0;
    }
    const std::string c = strip_gaps(cv.consensus_nt);
    memcpy(cons, c.data(), c.size());
    *cons_len = (uint32_t)c.size();
    if (mode != 1) return;
    corrected_pack_t cp = correct_read_pack(rs, msa, min_occ, gap_occ, err_ratio);
    std::vector<const read_t *> got(n, nullptr);
    for (const read_t &r : cp.reads) got[std::stoul(r.header)] = &r;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        out_off[i] = at;
        empty[i] = got[i] ? 0 : 1;
        if (!got[i]) continue;
        memcpy(out_seq + at, got[i]->seq.data(), got[i]->seq.size());
        memcpy(out_qual + at, got[i]->quality.data(), got[i]->seq.size());
        at += got[i]->seq.size();
    }
    out_off[n] = at;
}

// The graph every alignment of orc_poa_msa's loop is computed against (tests: which graph shape a pack really produces).  For
// k = 1 .. n-1, the graph after sequences 0 .. k-1 were added, by rank (= DP row - 1): aln_off[k-1] .. aln_off[k] index that
// graph's ranks in indeg[]; dist[] holds, rank after rank and in each node's in-edge order, rank(node) - rank(predecessor).
// aln_off [n], indeg and dist are malloc'd (orc_free); returns the length of dist, *n_nodes that of indeg.
uint64_t orc_poa_graph(const char *seqs, const uint64_t *off, uint32_t n, uint64_t **aln_off, uint32_t **indeg, uint32_t **dist, uint64_t *n_nodes) {
    poa_graph_t G;
    poa_engine_t eng;
    eng.simd = poa_simd_default();
    std::vector<uint64_t> ao(std::max<uint32_t>(n, 1), 0);
    std::vector<uint32_t> deg, dst;
    for (uint32_t k = 0; k < n; ++k) {
        const std::string s(seqs + off[k], seqs + off[k + 1]);
        if (k > 0) {
            std::vector<uint32_t> rank(G.nodes.size());
            for (size_t r = 0; r < G.rank_to_node.size(); ++r) rank[G.rank_to_node[r]] = (uint32_t)r;
            for (size_t r = 0; r < G.rank_to_node.size(); ++r) {
                const poa_node_t &nd = G.nodes[G.rank_to_node[r]];
                deg.push_back((uint32_t)nd.in_edges.size());
                for (uint32_t ei : nd.in_edges) dst.push_back((uint32_t)r - rank[G.edges[ei].begin]);
            }
            ao[k] = deg.size();
        }
        poa_alignment_t a = eng.align(s, G);
        G.add_alignment(a, s);
    }
    auto dump = [](const auto &v) {
        typedef typename std::decay<decltype(v)>::type::value_type T;
        T *p = (T *)malloc((v.size() + 1) * sizeof(T));
        memcpy(p, v.data(), v.size() * sizeof(T));
        return p;
    };
    *aln_off = dump(ao); *indeg = dump(deg); *dist = dump(dst);
    *n_nodes = deg.size();
    return dst.size();
}

// The facts kernel C's exact band is planned from, restated on the oracle's own graph and matrices (tests: on which side of
// the plan's comparisons a constructed pack sits).  For k = 1 .. n-1 of orc_poa_msa's loop, the graph after sequences 0 .. k-1:
// facts[5 (k-1) ..] = rows of the graph, its MSA columns C (ranks in topological order; a rank opens a column iff none of its node's
// aligned group has a smaller rank), L = |seqs[k]|, S = the best score of the full matrices (the scalar fill's), ordered = 1 iff every
// in-edge comes from a strictly earlier column.  cols (malloc'd, orc_free): the column (1-based) of every rank, graph after graph;
// returns its length (the sum of the graphs' rows).
uint64_t orc_poa_band_facts(const char *seqs, const uint64_t *off, uint32_t n, int64_t *facts, uint32_t **cols) {
    poa_graph_t G;
    poa_engine_t eng;                              // (scalar rows: their H is read below)
    std::vector<uint32_t> all;
    for (uint32_t k = 0; k < n; ++k) {
        const std::string s(seqs + off[k], seqs + off[k + 1]);
        poa_alignment_t a = eng.align(s, G);
        if (k > 0) {
            const size_t nv = G.nodes.size();
            std::vector<uint32_t> rank(nv), col(nv);
            for (size_t r = 0; r < nv; ++r) rank[G.rank_to_node[r]] = (uint32_t)r;
            uint32_t C = 0;
            for (size_t r = 0; r < nv; ++r) {
                const uint32_t v = G.rank_to_node[r];
                bool first = true;
                for (uint32_t m : G.nodes[v].aligned) if (rank[m] < r) first = false;
                if (first) ++C;
                col[v] = C;
                all.push_back(C);
            }
            bool ordered = true;
            for (const poa_edge_t &e : G.edges) if (col[e.begin] >= col[e.end]) ordered = false;
            int32_t S = 0;
            if (!s.empty()) for (int32_t h : eng.H) S = std::max(S, h);
            int64_t *f = facts + 5 * (size_t)(k - 1);
            f[0] = (int64_t)nv; f[1] = C; f[2] = (int64_t)s.size(); f[3] = S; f[4] = ordered ? 1 : 0;
        }
        G.add_alignment(a, s);
    }
    uint32_t *p = (uint32_t *)malloc((all.size() + 1) * sizeof(uint32_t));
    memcpy(p, all.data(), all.size() * sizeof(uint32_t));
    *cols = p;
    return all.size();
}

// poa_msa's loop with a deliberately WRONG row loop (tests: a constructed pack must notice).  Every alignment is computed against a
// copy of the graph in which the row loop's view of the in-edges is spoilt; the alignment is then added to the true graph.
// kind 1: a row's in-edges from the value-th on (0-based, in in-edge order) are not seen; 2: in-edges exactly `value` rows back are not
// seen; 3: in-edges `value` or more rows back are not seen; 4: a row without in-edge (not the first) takes the row before it as predecessor.
int64_t orc_poa_msa_blind(const char *seqs, const uint64_t *off, uint32_t n, int kind, uint32_t value, char *msa_out, uint64_t cap) {
    poa_graph_t G;
    poa_engine_t eng;
    eng.simd = poa_simd_default();
    for (uint32_t k = 0; k < n; ++k) {
        const std::string s(seqs + off[k], seqs + off[k + 1]);
        poa_graph_t M = G;
        std::vector<uint32_t> rank(M.nodes.size());
        for (size_t r = 0; r < M.rank_to_node.size(); ++r) rank[M.rank_to_node[r]] = (uint32_t)r;
        for (size_t v = 0; v < M.nodes.size(); ++v) {
            std::vector<uint32_t> &in = M.nodes[v].in_edges, kept;
            if (kind == 4) {
                if (in.empty() && rank[v] > 0) {
                    M.edges.push_back(poa_edge_t{M.rank_to_node[rank[v] - 1], (uint32_t)v, {}});
                    in.push_back((uint32_t)M.edges.size() - 1);
                }
                continue;
            }
            for (size_t i = 0; i < in.size(); ++i) {
                const uint32_t d = rank[v] - rank[M.edges[in[i]].begin];
                if ((kind == 1 && i >= value) || (kind == 2 && d == value) || (kind == 3 && d >= value)) continue;
                kept.push_back(in[i]);
            }
            in = kept;
        }
        poa_alignment_t a = eng.align(s, M);
        G.add_alignment(a, s);
    }
    std::vector<std::string> msa = G.msa();
    size_t W = msa.empty() ? 0 : msa[0].size();
    if (W * n > cap) return -1;
    for (uint32_t i = 0; i < n; ++i) memcpy(msa_out + (size_t)i * W, msa[i].data(), W);
    return (int64_t)W;
}

// poa_msa's loop with a deliberately WRONG scoring rule (tests: a pack of several alphabets must notice): two letters match when
// (c >> 1) & 3 is the same for both, which is how a score table indexed by those two bits sees them (T = U, A = @ = a, ...).  Every
// alignment is computed for the sequence and a copy of the graph with every letter replaced by "ACTG"[(c >> 1) & 3]; the alignment is
// then added to the true graph with the true letters, where nodes are told apart by byte as ever.
int64_t orc_poa_msa_table(const char *seqs, const uint64_t *off, uint32_t n, char *msa_out, uint64_t cap) {
    poa_graph_t G;
    poa_engine_t eng;
    eng.simd = poa_simd_default();
    auto twin = [](char c) { return "ACTG"[((unsigned char)c >> 1) & 3]; };
    for (uint32_t k = 0; k < n; ++k) {
        const std::string s(seqs + off[k], seqs + off[k + 1]);
        std::string t = s;
        for (char &c : t) c = twin(c);
        poa_graph_t M = G;
        for (auto &nd : M.nodes) nd.letter = twin(nd.letter);
        poa_alignment_t a = eng.align(t, M);
        G.dp_cells = M.dp_cells;
        G.add_alignment(a, s);
    }
    std::vector<std::string> msa = G.msa();
    size_t W = msa.empty() ? 0 : msa[0].size();
    if (W * n > cap) return -1;
    for (uint32_t i = 0; i < n; ++i) memcpy(msa_out + (size_t)i * W, msa[i].data(), W);
    return (int64_t)W;
}

void orc_free(void *p) { free(p); }

// AVX2 int16 row fill of the POA matrices (orc_poa.hpp); returns whether this CPU can run it.
int orc_set_poa_simd(int on) {
    poa_simd_default() = on != 0;
#if defined(__x86_64__)
    return __builtin_cpu_supports("avx2") ? 1 : 0;
#else
    return 0;
#endif
}

// Column-vote tie-break order (6 symbols), see orc_correct.hpp.
void orc_set_cv_order(const char *o) { set_cv_order(o); }

}  // extern "C"
