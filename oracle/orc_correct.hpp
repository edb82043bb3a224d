// ORACLE (test infrastructure, never shipped in the product path).
//
// CPU restatement of RATTLE's own half of `rattle correct` (everything in
// correct.cpp except the POA arithmetic, which is orc_poa.hpp).  Sequential
// (n_threads == 1) semantics: packs are processed in queue order and pack
// consensi are collected in pack order (the reference's multi-thread run
// collects them in completion order, correct.cpp:469 -- SURVEY B.24).
//
// Pinning: toyset/rna/output/consensi.fq + uncorrected.fq through
// tests/test_oracle_correct.py (see orc_poa.hpp header for the caveat).
#pragma once
#include <array>
#include <cmath>
#include <map>
#include <queue>
#include <string>
#include <vector>

#include "orc_cluster.hpp"
#include "orc_poa.hpp"

namespace orc {

typedef std::vector<std::string> msa_t;

inline char phred_symbol(double p) { return (char)(-10 * log10(p) + 33); }            // utils.cpp:6-8
inline double phred_err(char c) { double q = c - 33; return pow(10.0, -q / 10.0); }   // utils.cpp:10-13

// correct.cpp:32-92 (literal control flow, including the plain std::reverse of seq).
// erased (optional, tests): per row, the bases erased in the first phase (from the left end) and in the second (from the right).
inline void fix_msa_ends(read_set_t &reads, msa_t &aln, std::vector<std::array<uint32_t, 2>> *erased = nullptr) {
    if (erased) erased->assign(aln.size(), std::array<uint32_t, 2>{{0, 0}});
    for (size_t i = 0; i < aln.size(); ++i) {
        std::string &row = aln[i];
        bool reversed = false;
        bool again = true;
        while (again) {
            again = false;
            size_t pos = 0, end_pos = 0;
            while (pos < row.size()) {
                while (pos < row.size() && row[pos] == '-') ++pos;
                end_pos = pos;
                int gaps = 0, sz = 0;
                while (gaps < 4 && end_pos < row.size()) {
                    if (row[end_pos] == '-') ++gaps;
                    else { ++sz; gaps = 0; }
                    ++end_pos;
                }
                bool cut = false;
                if (sz < 10) {
                    while (end_pos < row.size() && row[end_pos] == '-') { ++end_pos; ++gaps; }
                    if (gaps >= 20) cut = true;
                }
                if (cut) {
                    for (size_t j = pos; j < end_pos; ++j) row[j] = '-';
                    reads[i].quality.erase(0, sz);
                    reads[i].seq.erase(0, sz);
                    if (erased) (*erased)[i][reversed ? 1 : 0] += (uint32_t)sz;
                    pos = end_pos;
                } else {
                    std::reverse(row.begin(), row.end());
                    std::reverse(reads[i].quality.begin(), reads[i].quality.end());
                    std::reverse(reads[i].seq.begin(), reads[i].seq.end());
                    if (!reversed) { reversed = true; again = true; }
                    break;
                }
            }
        }
    }
}

struct pos_info_t { double err; int occ; int total_occ; };

// Symbol slots in the reference's unordered_map<char,...> ITERATION order for the
// insertion sequence A,C,T,U,G,'-' on libstdc++ (correct.cpp:105-110): U - G T C A.
// The shipped toyset fixture (consensi.fq) was produced by an OLDER build whose order had
// A before C ("U-GTAC"): tests select it with set_cv_order() to pin the POA restatement
// against that fixture; the default is the order of the current reference source.
inline char *cv_order_storage() { static char o[7] = "U-GTCA"; return o; }
#define CV_ORDER (cv_order_storage())
inline void set_cv_order(const char *o) { for (int i = 0; i < 6; ++i) cv_order_storage()[i] = o[i]; }
inline int cv_slot(char c) {
    for (int i = 0; i < 6; ++i) if (CV_ORDER[i] == c) return i;
    fprintf(stderr, "oracle: unexpected MSA symbol %d\n", c); abort();
}

struct consensus_vector_t {
    std::vector<std::array<pos_info_t, 6>> nt_info;   // [column][slot]
    std::vector<char> consensus_nt;
};

// correct.cpp:94-193 with n_threads = 1 (single accumulation pass in row order).
inline consensus_vector_t generate_consensus_vector(const read_set_t &reads, const msa_t &aln) {
    consensus_vector_t cv;
    if (reads.size() == 0 || aln.size() == 0) return cv;
    size_t W = aln[0].size();
    cv.nt_info.assign(W, std::array<pos_info_t, 6>{});
    // :118-160: the worker accumulates into a local table, then adds it into the zeroed
    // global one (0.0 + x == x exactly, so one table is equivalent).
    for (size_t i = 0; i < reads.size(); ++i) {
        const std::string &row = aln[i];
        long seq_pos = -1;
        long qn = (long)reads[i].quality.size();
        for (size_t k = 0; k < row.size(); ++k) {
            char nt = row[k];
            double err_p = 0.0;
            if (nt != '-') { seq_pos++; err_p = phred_err(reads[i].quality[seq_pos]); }
            if (seq_pos >= 0 && seq_pos < qn) {
                pos_info_t &pi = cv.nt_info[k][cv_slot(nt)];
                pi.occ++;
                pi.err += err_p;
                if (seq_pos == qn - 1) seq_pos++;
            }
        }
    }
    cv.consensus_nt.resize(W);
    for (size_t k = 0; k < W; ++k) {                  // :171-190
        int max_occ = 0; char max_nt = 0;
        int tot = 0;
        for (int s = 0; s < 6; ++s) tot += cv.nt_info[k][s].occ;
        for (int s = 0; s < 6; ++s) {
            pos_info_t &pi = cv.nt_info[k][s];
            if (pi.occ > 0) { pi.total_occ += tot; pi.err /= double(pi.occ); }
            if (pi.occ > max_occ) { max_occ = pi.occ; max_nt = CV_ORDER[s]; }
        }
        if (max_nt == 0) max_nt = '-';
        cv.consensus_nt[k] = max_nt;
    }
    return cv;
}

struct corrected_pack_t {
    std::string consensus;
    read_set_t reads, uncorrected_reads;
};

// correct.cpp:196-309
inline corrected_pack_t correct_read_pack(const read_set_t &reads, const msa_t &aln, double min_occ, double gap_occ,
                                          double err_ratio) {
    consensus_vector_t cv = generate_consensus_vector(reads, aln);
    corrected_pack_t out;
    for (size_t i = 0; i < reads.size(); ++i) {
        const std::string &row = aln[i];
        long seq_pos = -1;
        long qn = (long)reads[i].quality.size();
        std::string res_read, res_qt;
        for (size_t k = 0; k < row.size(); ++k) {
            char nt = row[k];
            double err_p = 0.0;
            if (nt != '-') { seq_pos++; err_p = phred_err(reads[i].quality[seq_pos]); }
            if (seq_pos >= 0 && seq_pos < qn) {
                char cnt = cv.consensus_nt[k];
                const pos_info_t &ci = cv.nt_info[k][cv_slot(cnt)];
                double occ_ratio = double(ci.occ) / double(ci.total_occ);
                if (cnt == '-') {
                    if (nt != '-') {
                        if (occ_ratio >= gap_occ) { /* delete */ }
                        else { res_read += nt; res_qt += reads[i].quality[seq_pos]; }
                    }
                } else if (nt == '-') {
                    if (occ_ratio >= gap_occ) { res_read += cnt; res_qt += phred_symbol(ci.err); }
                } else if (nt == cnt) {
                    res_read += nt; res_qt += reads[i].quality[seq_pos];
                } else if (occ_ratio >= min_occ && err_ratio * err_p > ci.err) {
                    res_read += cnt; res_qt += phred_symbol(ci.err);
                } else {
                    res_read += nt; res_qt += reads[i].quality[seq_pos];
                }
                if (seq_pos == qn - 1) seq_pos++;
            }
        }
        if (res_read.size() > 0) out.reads.push_back(read_t{reads[i].header, res_read, "+", res_qt});
        else out.uncorrected_reads.push_back(reads[i]);
    }
    for (char c : cv.consensus_nt) if (c != '-') out.consensus += c;
    return out;
}

struct correction_results_t { read_set_t corrected, uncorrected, consensi; };

struct correct_counters_t { uint64_t dp_cells = 0, packs = 0, alignments = 0; };

inline std::vector<std::string> split_string(const std::string &s, char d) {   // correct.cpp:20-30
    std::vector<std::string> out;
    size_t b = 0;
    if (s.empty()) return out;
    while (true) {
        size_t e = s.find(d, b);
        if (e == std::string::npos) { out.push_back(s.substr(b)); break; }
        out.push_back(s.substr(b, e - b));
        b = e + 1;
        if (b == s.size()) break;     // getline drops a trailing empty token
    }
    return out;
}

inline std::string strip_gaps(const std::vector<char> &v) {
    std::string s;
    for (char c : v) if (c != '-') s += c;
    return s;
}

// correct.cpp:311-563, n_threads = 1.
inline correction_results_t correct_reads(const cluster_set_t &clusters, read_set_t &reads, double min_occ, double gap_occ,
                                          double err_ratio, int split, int min_reads, const std::vector<std::string> &labels,
                                          correct_counters_t *cc = nullptr,
                                          const std::map<int, std::vector<int>> *pack_order = nullptr) {
    struct pack_t { int cid; read_set_t reads; };
    std::queue<pack_t> pending;
    correction_results_t R;
    bool gene_mode = clusters[0].main_seq.gene_id == -1;       // :322
    int cid = 0;
    for (auto &tc : clusters) {                                // :328-370
        int n_files = ((int)tc.seqs.size() - 1) / split + 1;
        int gid = tc.main_seq.gene_id;
        for (int nf = 0; nf < n_files; ++nf) {
            read_set_t creads;
            for (size_t j = nf; j < tc.seqs.size(); j += n_files) {
                const cseq_t &ts = tc.seqs[j];
                read_t &r = reads[ts.seq_id];
                if (ts.rev) {
                    r.seq = reverse_complement(r.seq);
                    std::reverse(r.quality.begin(), r.quality.end());
                }
                if (gid == -1) r.header += ",gene_cluster_" + std::to_string(cid);
                else r.header += ",gene_cluster_" + std::to_string(gid) + ",transcript_cluster_" + std::to_string(cid);
                creads.push_back(r);
            }
            if ((int)creads.size() > min_reads) pending.push(pack_t{cid, creads});
            else for (auto &r : creads) R.uncorrected.push_back(r);
        }
        ++cid;
    }
    std::vector<read_set_t> consensi(clusters.size());
    while (!pending.empty()) {                                 // :379-476
        pack_t pack = pending.front();
        pending.pop();
        read_set_t creads = pack.reads;
        std::vector<std::string> seqs;
        for (auto &r : creads) seqs.push_back(r.seq);
        uint64_t cells = 0;
        msa_t msa = poa_msa(seqs, &cells);
        fix_msa_ends(creads, msa);
        corrected_pack_t cp = correct_read_pack(creads, msa, min_occ, gap_occ, 30.0);
        read_set_t corrected = cp.reads;
        for (auto &r : corrected) R.corrected.push_back(r);
        for (auto &r : cp.uncorrected_reads) R.uncorrected.push_back(r);
        sort_read_set(corrected);                              // :427
        seqs.clear();
        for (auto &r : corrected) seqs.push_back(r.seq);
        msa = poa_msa(seqs, &cells);
        fix_msa_ends(corrected, msa);
        consensus_vector_t cv = generate_consensus_vector(corrected, msa);
        std::string consensus = strip_gaps(cv.consensus_nt);
        if (cc) { cc->dp_cells += cells; cc->packs++; cc->alignments += creads.size() + corrected.size(); }
        std::vector<std::string> labelset;                     // :453-469
        std::string gid;
        for (auto &r : creads) {
            int index = (int)r.header.find_first_of(",");
            int i2 = (int)r.header.substr(index + 1).find_first_of(",");
            labelset.push_back(r.header.substr(index + 1, i2));
            index = (int)r.header.find("gene_cluster");
            gid = std::to_string(std::stoi(r.header.substr(index + 13)));
        }
        std::string label_result;
        for (auto &l : labels)
            label_result = label_result + " " + l + ":" + std::to_string(std::count(labelset.begin(), labelset.end(), l));
        consensi[pack.cid].push_back(read_t{gid + "," + std::to_string(creads.size()) + "," + label_result, consensus, "+",
                                            std::string(consensus.size(), 'K')});
    }
    // The reference's workers push pack consensi in COMPLETION order (:469); a given order (a permutation of
    // the cluster's queued packs) reproduces one such run.  Default: pack order (n_threads == 1).
    if (pack_order)
        for (auto &po : *pack_order) {
            read_set_t &it = consensi[po.first];
            if (po.second.size() != it.size()) { fprintf(stderr, "oracle: pack order of cluster %d has %zu entries for %zu packs\n", po.first, po.second.size(), it.size()); abort(); }
            read_set_t re;
            for (int k : po.second) re.push_back(it[k]);
            it.swap(re);
        }
    cid = 0;
    for (auto &it : consensi) {                                // :489-556
        int total_reads = 0, gid = 0;
        std::vector<int> label_counts(labels.size());
        for (auto &rit : it) {
            auto num = split_string(rit.header, ',');
            gid = std::stoi(num[0]);
            total_reads += std::stoi(num[1]);
            int i = 0;
            for (auto &l : labels) {
                size_t idx = rit.header.find(l);
                if (idx != std::string::npos) {
                    std::string sub = rit.header.substr(idx + 1);
                    size_t c = sub.find_first_of(":");
                    label_counts[i] += std::stoi(sub.substr(c + 1));
                }
                ++i;
            }
        }
        std::string labels_result;
        for (size_t i = 0; i < labels.size(); ++i) labels_result += labels[i] + ":" + std::to_string(label_counts[i]) + ",";
        std::string head = gene_mode
            ? "@gene_cluster_" + std::to_string(cid) + " reads=" + std::to_string(total_reads) + " labels=" + labels_result
            : "@transcript_cluster_" + std::to_string(cid) + " gene_cluster_" + std::to_string(gid) + " reads=" +
                  std::to_string(total_reads) + " labels=" + labels_result;
        if (it.size() > 1) {
            std::vector<std::string> seqs;
            for (auto &r : it) seqs.push_back(r.seq);
            uint64_t cells = 0;
            msa_t msa = poa_msa(seqs, &cells);
            if (cc) { cc->dp_cells += cells; cc->alignments += it.size(); }
            fix_msa_ends(it, msa);
            consensus_vector_t cv = generate_consensus_vector(it, msa);
            std::string consensus = strip_gaps(cv.consensus_nt);
            R.consensi.push_back(read_t{head, consensus, "+", std::string(consensus.size(), 'K')});
        } else if (it.size() > 0) {
            R.consensi.push_back(read_t{head, it[0].seq, "+", it[0].quality});
        }
        ++cid;
    }
    return R;
}

}  // namespace orc
