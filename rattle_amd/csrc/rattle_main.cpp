// `rattle` command line: drop-in for `rattle cluster` (/root/reference/main.cpp:133-324),
// `rattle correct` (:325-412) and `rattle polish` (:612-762) over librattle_hip.so's C ABI.
// Same flags and defaults, same `clusters.out` (hps stream) and FASTQ outputs.  Host C++ only:
// every compute step goes through include/rattle_hip.h.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <chrono>
#include <cmath>

#include "../../include/rattle_hip.h"

// RATTLE_TIMING=1: wall time of the CLI's own phases on stderr (the library prints its phases the same way)
struct cli_timer {
    const char *name;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit cli_timer(const char *n) : name(n) {}
    ~cli_timer() {
        static const bool on = getenv("RATTLE_TIMING") != nullptr;
        if (on) fprintf(stderr, "[rattle cli] %-26s %8.1f ms\n", name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// An output file of known size: the text is laid out by record offsets, formatted by all threads into an UNinitialised
// buffer (the page faults spread over the threads; a zero-filled std::vector would touch the 2 GB once more, alone), and
// written with one pwrite stream per thread.
struct sized_output {
    std::string path;
    char *p = nullptr;
    size_t size = 0;
    sized_output(const std::string &path_, size_t n) : path(path_), size(n) {
        p = (char *)malloc(n ? n : 1);
        if (!p) { fprintf(stderr, "Error: out of memory for %s\n", path.c_str()); exit(EXIT_FAILURE); }
    }
    ~sized_output() { free(p); }
    bool finish() {
        const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) return false;
        std::atomic<bool> ok(true);
        const size_t piece = 32u << 20;
        const size_t n_pieces = (size + piece - 1) / piece;
        std::atomic<size_t> next(0);
        auto work = [&]() {
            for (size_t i = next++; i < n_pieces && ok; i = next++) {
                size_t at = i * piece;
                const size_t end = std::min(size, at + piece);
                while (at < end) {
                    const ssize_t w = pwrite(fd, p + at, end - at, (off_t)at);
                    if (w <= 0) { ok = false; break; }
                    at += (size_t)w;
                }
            }
        };
        const size_t T = std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)std::thread::hardware_concurrency(), n_pieces}));
        std::vector<std::thread> th;
        for (size_t t = 1; t < T; ++t) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
        return (close(fd) == 0) && ok;
    }
};

namespace {

struct read_t { std::string header, seq, ann, quality; };      // fasta.hpp:7-12
typedef std::vector<read_t> read_set_t;
struct cseq_t { int seq_id; bool rev; int gene_id; };            // cluster.hpp:10-13
struct cluster_t { cseq_t main_seq; std::vector<cseq_t> seqs; };
typedef std::vector<cluster_t> cluster_set_t;

[[noreturn]] void die(const std::string &m) { std::cerr << m << std::endl; exit(EXIT_FAILURE); }
void chk(int rc) { if (rc != 0) die(std::string("\nError: ") + rattle_hip_last_error()); }

// ---- argument parsing: --name v, --name=v, -n v, -nv, flags (argagg behaviour used by main.cpp) ----
struct opt_def { const char *key; std::vector<std::string> names; bool has_arg; };
struct args_t {
    std::map<std::string, std::string> v;
    bool has(const std::string &k) const { return v.count(k) != 0; }
    std::string str(const std::string &k, const std::string &d) const { auto i = v.find(k); return i == v.end() ? d : i->second; }
    int i(const std::string &k, int d) const { auto it = v.find(k); return it == v.end() ? d : std::stoi(it->second); }
    double d(const std::string &k, double dv) const { auto it = v.find(k); return it == v.end() ? dv : std::stod(it->second); }
};

args_t parse(int argc, char **argv, const std::vector<opt_def> &defs) {
    args_t a;
    for (int i = 2; i < argc; ++i) {
        std::string tok = argv[i], val;
        bool has_val = false;
        if (tok.rfind("--", 0) == 0) {
            size_t eq = tok.find('=');
            if (eq != std::string::npos) { val = tok.substr(eq + 1); tok = tok.substr(0, eq); has_val = true; }
        } else if (tok.size() > 2 && tok[0] == '-') {
            val = tok.substr(2); tok = tok.substr(0, 2); has_val = true;
        }
        const opt_def *d = nullptr;
        for (auto &o : defs) for (auto &n : o.names) if (n == tok) d = &o;
        if (!d) die("unknown option \"" + tok + "\"");
        if (!d->has_arg) { a.v[d->key] = "1"; continue; }
        if (!has_val) { if (i + 1 >= argc) die("option \"" + tok + "\" needs an argument"); val = argv[++i]; }
        a.v[d->key] = val;
    }
    return a;
}

std::vector<std::string> split_string(const std::string &s, char d) {            // correct.cpp:20-30
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string t;
    while (getline(ss, t, d)) out.push_back(t);
    return out;
}

// the name of a record: the first token of its header, without the '@' / '>' (what api._first_token returns)
std::string record_name(const char *p, size_t n) {
    const char *e = p + n;
    if (p < e && (*p == '@' || *p == '>')) ++p;
    while (p < e && (*p == ' ' || *p == '\t')) ++p;
    const char *t = p;
    while (t < e && *t != ' ' && *t != '\t') ++t;
    return std::string(p, t - p);
}
std::string record_name(const std::string &h) { return record_name(h.data(), h.size()); }

std::string g17(double x) { char b[40]; snprintf(b, sizeof b, "%.17g", x); return b; }   // a double that reads back exactly

void write_text(const std::string &path, const std::string &text) {
    std::ofstream f(path);
    f << text;
    f.close();
    if (!f) die("Error: cannot write " + path);
}

// --report / --support: made on one device
void one_device_only(const args_t &a, const char *flag, const char *what) {
    if (a.has(flag) && a.has("devices") && split_string(a.str("devices", ""), ',').size() > 1)
        die(std::string("\nError: --") + flag + " cannot be combined with --devices naming more than one device: the " + what + " is made on one device\n");
}

// --count-pass auto|seed|search|index -> 0..3 (rattle_assign_params::count_pass; the names are what RATTLE_PAIR_COUNT takes)
int count_pass_of(const std::string &form, const char *usage) {
    const char *forms[] = {"auto", "seed", "search", "index"};
    for (int i = 0; i < 4; ++i) if (form == forms[i]) return i;
    std::cerr << "ERROR: --count-pass takes auto, seed, search or index (got '" << form << "')\nusage: " << usage;
    exit(EXIT_FAILURE);
}

std::string output_dir(const args_t &a) {
    const std::string dir = a.str("output", ".");
    if (a.has("output") && access(dir.c_str(), F_OK)) die("\nOutput folder doesn't exit. Please create it first. \n");
    return dir;
}

rattle_cluster_params default_cluster_params() {                                  // main.cpp:133-324, `cluster`'s defaults
    rattle_cluster_params P;
    P.t_s = 0.2; P.t_v = 1000000; P.bv_threshold = 0.4; P.min_bv_threshold = 0.2; P.bv_falloff = 0.05;
    P.min_reads_cluster = 0; P.use_hc = 0; P.repr_percentile = 0.15; P.is_rna = 0;
    return P;
}
rattle_correct_params default_correct_params() {                                  // main.cpp:325-412, `correct`'s defaults
    rattle_correct_params P;
    memset(&P, 0, sizeof(P));
    P.min_occ = 0.3; P.gap_occ = 0.3; P.err_ratio = 30.0; P.split = 200; P.min_reads = 5; P.n_threads = 0;
    return P;
}

// ---- input of `polish`: the records of a FASTQ file (4 lines each), fasta.cpp:207-270 --------------
void for_each_fastq_record(const std::string &file, const std::function<void(const std::string &, const std::string &, const std::string &, const std::string &)> &f) {
    // whole file in memory, lines by memchr (std::getline was the slowest part of a run once the kernels were fast);
    // same line semantics: '\n' separated, a final line without one counts, DOS endings detected on line 1
    FILE *fp = fopen(file.c_str(), "rb");
    if (!fp) return;
    std::string buf;
    {
        fseek(fp, 0, SEEK_END);
        const long sz = ftell(fp);
        fseek(fp, 0, SEEK_SET);
        buf.resize(sz > 0 ? (size_t)sz : 0);
        size_t got = 0;
        while (got < buf.size()) { const size_t n = fread(&buf[got], 1, buf.size() - got, fp); if (n == 0) break; got += n; }
        buf.resize(got);
        fclose(fp);
    }
    std::string fld[4];
    bool dos = false, first = true;
    int id = 0;
    size_t pos = 0;
    while (pos < buf.size()) {
        const char *nl = (const char *)memchr(buf.data() + pos, '\n', buf.size() - pos);
        size_t end = nl ? (size_t)(nl - buf.data()) : buf.size();
        size_t len = end - pos;
        if (first) { dos = len > 0 && buf[end - 1] == '\r'; first = false; }
        if (dos && len > 0) --len;
        fld[id].assign(buf.data() + pos, len);
        pos = end + 1;
        if (++id == 4) { f(fld[0], fld[1], fld[2], fld[3]); id = 0; }
    }
}

void write_fastq_file(const read_set_t &reads, const std::string &file) {        // fasta.cpp:436-445
    std::ofstream f(file);
    for (auto &r : reads) f << r.header << "\n" << r.seq << "\n" << r.ann << "\n" << r.quality << "\n";
}

// ---- clusters.out: hps stream of cluster_set_t (cluster.hpp:15-18,30-33; grammar SURVEY 5) ---------
void put_uvarint(std::string &o, uint64_t x) { while (x >= 0x80) { o.push_back((char)((x & 0x7F) | 0x80)); x >>= 7; } o.push_back((char)x); }
void put_svarint(std::string &o, int32_t x) { put_uvarint(o, (uint32_t)((x << 1) ^ (x >> 31))); }

void write_clusters(const cluster_set_t &cs, const std::string &path) {
    std::string o;
    put_uvarint(o, cs.size());
    auto cseq = [&o](const cseq_t &c) { put_svarint(o, c.seq_id); o.push_back(c.rev ? 1 : 0); put_svarint(o, c.gene_id); };
    for (auto &c : cs) { cseq(c.main_seq); put_uvarint(o, c.seqs.size()); for (auto &s : c.seqs) cseq(s); }
    std::ofstream f(path, std::ofstream::binary);
    f.write(o.data(), (std::streamsize)o.size());
}

bool decode_clusters(const std::string &b, int fields, cluster_set_t &out) {
    size_t p = 0;
    bool ok = true;
    auto uv = [&]() -> uint64_t {
        uint64_t x = 0; int s = 0;
        while (true) {
            if (p >= b.size() || s > 63) { ok = false; return 0; }
            uint8_t c = (uint8_t)b[p++];
            x |= (uint64_t)(c & 0x7F) << s;
            if (!(c & 0x80)) return x;
            s += 7;
        }
    };
    auto sv = [&]() -> int32_t { uint32_t z = (uint32_t)uv(); return (int32_t)((z >> 1) ^ (~(z & 1) + 1)); };
    auto cseq = [&]() -> cseq_t {
        cseq_t c{0, false, -1};
        c.seq_id = sv();
        if (p >= b.size()) { ok = false; return c; }
        uint8_t r = (uint8_t)b[p++];
        if (r > 1) ok = false;
        c.rev = r != 0;
        if (fields == 3) c.gene_id = sv();
        return c;
    };
    out.clear();
    uint64_t n = uv();
    for (uint64_t i = 0; ok && i < n; ++i) {
        cluster_t c;
        c.main_seq = cseq();
        uint64_t m = uv();
        for (uint64_t j = 0; ok && j < m; ++j) c.seqs.push_back(cseq());
        out.push_back(c);
    }
    return ok && p == b.size();
}

cluster_set_t read_clusters(const std::string &path) {            // current 3-field layout, else the old 2-field one
    std::ifstream in(path, std::ifstream::binary);
    if (!in) die("\nError: clusters file not found! \n");
    std::string b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    cluster_set_t cs;
    if (decode_clusters(b, 3, cs) || decode_clusters(b, 2, cs)) return cs;
    die("\nError: clusters file is not an hps cluster stream\n");
}

// ---- ingest for `cluster` / `correct` (fasta.cpp:7-31,207-370, main.cpp:16-112) -----------------------
// The reference reads line by line into four std::string per record and inflates .gz inputs into a sibling file first.  Here
// a record is four spans into the file's bytes: a plain file is mapped, a .gz one inflated in memory (the sibling file is
// only written with --write-unzipped), records are found with memchr, and the concatenated base / quality buffers the library
// takes are gathered from the spans in parallel.  Same semantics: '\n' separated lines, a last line without one counts, DOS
// endings detected on the first line, FASTA sequence lines joined and upper-cased, quality '~' for FASTA.
struct span { const char *p; uint32_t n; };
std::string record_name(const span &h) { return record_name(h.p, h.n); }
struct read_table {
    std::vector<std::unique_ptr<std::string>> pools;       // owned bytes (inflated input, joined FASTA sequences, label suffixes)
    std::vector<std::pair<void *, size_t>> maps;           // mapped files
    std::vector<span> header, seq, ann, qual;
    std::vector<uint32_t> label;                           // 0: none, else 1 + index into labels
    std::vector<std::string> labels;                       // "," + label
    size_t n() const { return seq.size(); }
    std::string head(size_t i) const { return std::string(header[i].p, header[i].n) + (label[i] ? labels[label[i] - 1] : std::string()); }
    ~read_table() { for (auto &m : maps) munmap(m.first, m.second); }
    read_table() = default;
    read_table(const read_table &) = delete;
    read_table &operator=(const read_table &) = delete;
};

template <typename F>
void parallel_chunks(size_t n, F f) {                     // f(begin, end) on host threads
    const size_t T = std::max<size_t>(1, std::min<size_t>(std::thread::hardware_concurrency(), (n + 4095) / 4096));
    if (T <= 1) { f(0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t) th.emplace_back([=] { f(n * t / T, n * (t + 1) / T); });
    for (auto &x : th) x.join();
}

// bytes of an input file: mapped, or inflated in memory for .gz (main.cpp:35-57 decides by extension)
void file_bytes(read_table &T, std::string &filename, bool &fastq, bool write_unzipped, const char *&data, size_t &size) {
    if (access(filename.c_str(), F_OK)) die("\nError: Input file not found! \n");
    int index = (int)filename.find_last_of(".");
    std::string ext = filename.substr(index + 1);
    bool gz = false;
    std::string inner = filename;
    if (ext == "gz") {
        gz = true;
        inner = filename.substr(0, index);
        index = (int)inner.find_last_of(".");
        ext = inner.substr(index + 1);
    }
    if (ext == "fq" || ext == "fastq") fastq = true;
    else if (ext == "fasta" || ext == "fa") fastq = false;
    else die("\nError: Input file format incorrect! Please use fasta/fastq file. \n");
    if (gz) {
        std::cerr << "Start decompressing file" << std::endl;
        gzFile in = gzopen(filename.c_str(), "rb");
        if (!in) die("Error: Failed to decompress the file");
        gzbuffer(in, 1 << 20);
        std::unique_ptr<std::string> buf(new std::string());
        size_t got = 0;
        buf->resize(64u << 20);
        int k;
        while ((k = gzread(in, &(*buf)[got], (unsigned)std::min<size_t>(buf->size() - got, 1u << 30))) > 0) {
            got += (size_t)k;
            if (buf->size() - got < (16u << 20)) buf->resize(buf->size() * 2);
        }
        gzclose(in);
        buf->resize(got);
        if (write_unzipped) {                           // the reference's side effect (fasta.cpp:7-31): the inflated sibling file
            FILE *f = fopen(inner.c_str(), "wb");
            if (!f) die("Error: Failed to decompress the file");
            fwrite(buf->data(), 1, buf->size(), f);
            fclose(f);
        }
        std::cerr << "Decompressing file Complete" << std::endl;
        data = buf->data(); size = buf->size();
        T.pools.push_back(std::move(buf));
        return;
    }
    const int fd = open(filename.c_str(), O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) die("\nError: Input file not found! \n");
    size = (size_t)st.st_size;
    data = "";
    if (size) {
        void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
        if (m == MAP_FAILED) die("Error: cannot map " + filename);
        (void)madvise(m, size, MADV_SEQUENTIAL);
        T.maps.emplace_back(m, size);
        data = (const char *)m;
    }
    close(fd);
}

// all records of the input files, in file order (main.cpp:66-112: `correct`, `cluster_summary`, ... read everything)
void read_table_inputs(read_table &T, const std::vector<std::string> &files, const std::vector<std::string> &labels, bool write_unzipped) {
    if (!labels.empty() && labels.size() != files.size()) die("\nError: Number of input files and number of label files do not match\n");
    for (auto &l : labels) T.labels.push_back("," + l);
    uint32_t sample = 0;
    for (std::string fn : files) {
        bool fastq = true;
        const char *d; size_t sz;
        file_bytes(T, fn, fastq, write_unzipped, d, sz);
        const uint32_t lab = labels.empty() ? 0u : sample + 1;
        if (fastq) {
            span fld[4];
            bool dos = false, first = true;
            int id = 0;
            size_t pos = 0;
            while (pos < sz) {
                const char *nl = (const char *)memchr(d + pos, '\n', sz - pos);
                const size_t end = nl ? (size_t)(nl - d) : sz;
                size_t len = end - pos;
                if (first) { dos = len > 0 && d[end - 1] == '\r'; first = false; }
                if (dos && len > 0) --len;
                fld[id] = span{d + pos, (uint32_t)len};
                pos = end + 1;
                if (++id == 4) { T.header.push_back(fld[0]); T.seq.push_back(fld[1]); T.ann.push_back(fld[2]); T.qual.push_back(fld[3]); T.label.push_back(lab); id = 0; }
            }
        } else {
            // FASTA: header + joined, upper-cased sequence lines (fasta.cpp:60,131); quality '~' x length
            std::unique_ptr<std::string> pool(new std::string());
            pool->reserve(sz + 16);
            struct rec { size_t h0; uint32_t hn; size_t s0, s1; };
            std::vector<rec> recs;
            bool dos = false, first = true, have = false;
            rec cur{0, 0, 0, 0};
            size_t pos = 0;
            while (pos < sz) {
                const char *nl = (const char *)memchr(d + pos, '\n', sz - pos);
                const size_t end = nl ? (size_t)(nl - d) : sz;
                size_t len = end - pos;
                if (first) { dos = len > 0 && d[end - 1] == '\r'; first = false; }
                if (dos && len > 0) --len;
                if (len) {
                    if (d[pos] == '>') {
                        if (have) { cur.s1 = pool->size(); recs.push_back(cur); }
                        cur = rec{pos, (uint32_t)len, pool->size(), 0}; have = true;
                    } else {
                        for (size_t t = 0; t < len; ++t) pool->push_back((char)toupper((unsigned char)d[pos + t]));
                    }
                }
                pos = end + 1;
            }
            if (have) { cur.s1 = pool->size(); recs.push_back(cur); }
            size_t longest = 0;
            for (auto &r : recs) longest = std::max(longest, r.s1 - r.s0);
            std::unique_ptr<std::string> tilde(new std::string(longest, '~'));
            for (auto &r : recs) {
                T.header.push_back(span{d + r.h0, r.hn}); T.seq.push_back(span{pool->data() + r.s0, (uint32_t)(r.s1 - r.s0)});
                T.ann.push_back(span{"", 0}); T.qual.push_back(span{tilde->data(), (uint32_t)(r.s1 - r.s0)}); T.label.push_back(lab);
            }
            T.pools.push_back(std::move(pool)); T.pools.push_back(std::move(tilde));
        }
        ++sample;
    }
}

// the same as owned strings, for the host-only modes (the reference's side effect included: a .gz input is also inflated next to itself)
read_set_t read_inputs(const std::vector<std::string> &files, const std::vector<std::string> &labels) {
    read_table T;
    read_table_inputs(T, files, labels, true);
    auto str = [](const span &x) { return std::string(x.p, x.n); };
    read_set_t reads;
    for (size_t i = 0; i < T.n(); ++i) reads.push_back(read_t{T.head(i), str(T.seq[i]), str(T.ann[i]), str(T.qual[i])});
    return reads;
}

// concatenated bases (and qualities, padded with '!' / cut to the sequence length) of the records `ids` in that order
// bytes that are filled right away by all threads: no zero fill by one thread first (a GB-sized std::vector costs 0.1 s that way)
struct byte_buf {
    std::unique_ptr<uint8_t[]> p;
    void resize(size_t n) { p.reset(new uint8_t[n]); }
    uint8_t *data() const { return p.get(); }
};

void gather_reads(const read_table &T, const std::vector<uint32_t> &ids, byte_buf &cat, byte_buf *qcat, std::vector<uint64_t> &off) {
    const size_t n = ids.size();
    off.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + T.seq[ids[i]].n;
    cat.resize(off[n] + 1);
    if (qcat) qcat->resize(off[n] + 1);
    parallel_chunks(n, [&](size_t b, size_t e) {
        for (size_t i = b; i < e; ++i) {
            const span sq = T.seq[ids[i]];
            memcpy(cat.data() + off[i], sq.p, sq.n);
            if (qcat) {
                const span q = T.qual[ids[i]];
                const uint32_t m = std::min(q.n, sq.n);
                memcpy(qcat->data() + off[i], q.p, m);
                if (m < sq.n) memset(qcat->data() + off[i] + m, '!', sq.n - m);
            }
        }
    });
}

// ---- one job over several GPUs of the node: --devices 0,1,... --------------------------------------------------
// One host thread per device, each with its own context; every thread makes the same library calls and the library shards
// the work (candidates of a seed batch, --iso gene clusters, `correct` packs; include/rattle_hip.h).  The exchange is RCCL
// over xGMI; --host-exchange swaps in an in-process all-gather on host buffers (no RCCL needed; also lets several ranks
// share one device, which RCCL refuses).
struct host_exchange {
    int n = 1;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    std::vector<const void *> send;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t g = generation;
        if (++arrived == n) { arrived = 0; ++generation; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != g; });
    }
};
struct rank_user { host_exchange *X; int rank; };
int host_allgatherv(void *user, const void *send, uint64_t, void *recv, const uint64_t *recv_bytes) {
    rank_user *u = (rank_user *)user;
    host_exchange &X = *u->X;
    X.send[u->rank] = send;
    X.barrier();                                   // every rank has published its piece
    uint64_t at = 0;
    for (int r = 0; r < X.n; ++r) { if (recv_bytes[r]) memcpy((char *)recv + at, X.send[r], recv_bytes[r]); at += recv_bytes[r]; }
    X.barrier();                                   // every rank has copied: the pieces may be released
    return 0;
}

struct device_team {
    std::vector<int> devs;
    std::vector<rattle_ctx *> ctx;
    host_exchange hx;
    std::vector<rank_user> users;
    int n() const { return (int)devs.size(); }
    // fn(rank, ctx) on every rank at once (rank 0 on the calling thread)
    void run(const std::function<void(int, rattle_ctx *)> &fn) {
        std::vector<std::thread> th;
        for (int r = 1; r < n(); ++r) th.emplace_back([&, r] { fn(r, ctx[r]); });
        fn(0, ctx[0]);
        for (auto &t : th) t.join();
    }
    void open(const args_t &a) {
        if (a.has("devices")) for (auto &t : split_string(a.str("devices", ""), ',')) devs.push_back(std::stoi(t));
        else devs.push_back(a.i("device", 0));
        if (devs.empty()) die("\nError: --devices needs a list of device indices\n");
        ctx.assign(devs.size(), nullptr);
        const bool host = a.has("host-exchange");
        uint8_t id[RATTLE_COMM_ID_BYTES] = {0};
        if (n() > 1 && !host) chk(rattle_hip_comm_unique_id(id));
        hx.n = n(); hx.send.assign(devs.size(), nullptr);
        users.resize(devs.size());
        for (int r = 0; r < n(); ++r) users[r] = rank_user{&hx, r};
        run([&](int r, rattle_ctx *) {
            chk(rattle_hip_ctx_create(devs[r], &ctx[r]));
            if (n() > 1) chk(host ? rattle_hip_set_exchange(ctx[r], r, n(), host_allgatherv, &users[r]) : rattle_hip_comm_init(ctx[r], r, n(), id));
        });
        if (n() > 1) std::cerr << "One job over " << n() << " devices (" << (host ? "host exchange" : "RCCL") << ")" << std::endl;
    }
    void close() { for (auto *c : ctx) rattle_hip_ctx_destroy(c); ctx.clear(); }
};

// ---- device calls --------------------------------------------------------------------------------
cluster_set_t to_set(rattle_cluster_set *cs) {
    cluster_set_t out(cs->n_clusters);
    for (uint32_t c = 0; c < cs->n_clusters; ++c) {
        out[c].main_seq = cseq_t{cs->main_id[c], cs->main_rev[c] != 0, -1};
        for (uint32_t i = cs->offsets[c]; i < cs->offsets[c + 1]; ++i) out[c].seqs.push_back(cseq_t{cs->member_id[i], cs->member_rev[i] != 0, -1});
    }
    rattle_hip_cluster_set_free(cs);
    return out;
}

// context creation (HIP start-up, ~0.5 s) and, for `correct`, the POA arena allocation (seconds for > 100 GB) run on a helper
// thread while the main thread reads the input
struct team_opener {
    std::thread th;
    void start(device_team &t, const args_t &a, uint64_t arena_hint) {
        th = std::thread([&t, &a, arena_hint] {
            t.open(a);
            if (arena_hint) t.run([&](int, rattle_ctx *c) { (void)rattle_hip_reserve_arena(c, arena_hint); });
        });
    }
    void wait() { if (th.joinable()) th.join(); }
    ~team_opener() { wait(); }
};

// the clusters' members as rattle_hip_correct_reads takes them
void flatten_members(const cluster_set_t &clusters, std::vector<uint32_t> &coff, std::vector<int32_t> &mid, std::vector<uint8_t> &mrev) {
    coff.assign(1, 0);
    for (auto &c : clusters) {
        for (auto &s : c.seqs) { mid.push_back(s.seq_id); mrev.push_back(s.rev ? 1 : 0); }
        coff.push_back((uint32_t)mid.size());
    }
}

// record i of a correction's consensi under the header the mode gives it
read_t consensus_record(const rattle_read_set &S, uint32_t i, const std::string &header) {
    return read_t{header, std::string(S.seq + S.off[i], S.seq + S.off[i + 1]), "+", std::string(S.qual + S.off[i], S.qual + S.off[i + 1])};
}

uint64_t input_bytes(const std::vector<std::string> &files) {
    uint64_t tot = 0;
    for (auto &f : files) { struct stat st; if (stat(f.c_str(), &st) == 0) tot += (uint64_t)st.st_size * (f.size() > 3 && f.substr(f.size() - 3) == ".gz" ? 4 : 1); }
    return tot;
}

// ---- `rattle cluster` ----------------------------------------------------------------------------------------------------
struct cluster_job {
    args_t a;
    int k = 10, iso_k = 11;
    bool is_rna = false, want_report = false;
    std::string outdir;
    device_team team;
    team_opener opener;                           // opens `team` behind the reading of the input
    read_table T;
    std::vector<uint32_t> order;                  // processing position -> record index (= the reference's `ann`)
    byte_buf cat;                                 // the bases of the reads in processing order
    std::vector<uint64_t> off;                    // [n + 1] their offsets in `cat`
    rattle_cluster_params P = default_cluster_params();
    cluster_set_t clusters;                       // over processing positions: the gene clusters, then with --iso the isoform clusters
    std::string report_text = "level\tpass\tbv_threshold\tabsorbed\tinto\tstrand\tbases\thc_bases\tmin_len\tscore\tvariance\n";
    std::unique_ptr<cli_timer> t_out;
    void options(int argc, char **argv) {
        a = parse(argc, argv, {
            {"help", {"-h", "--help"}, false}, {"input", {"-i", "--input"}, true}, {"label", {"-l", "--label"}, true},
            {"output", {"-o", "--output"}, true}, {"threads", {"-t", "--threads"}, true}, {"kmer_size", {"-k", "--kmer-size"}, true},
            {"t_s", {"-s", "--score-threshold"}, true}, {"t_v", {"-v", "--max-variance"}, true}, {"iso", {"--iso"}, false},
            {"iso_kmer_size", {"--iso-kmer-size"}, true}, {"iso_t_s", {"--iso-score-threshold"}, true},
            {"iso_t_v", {"--iso-max-variance"}, true}, {"bv_threshold", {"-B", "--bv-start-threshold"}, true},
            {"bv_min_threshold", {"-b", "--bv-end-threshold"}, true}, {"bv_falloff", {"-f", "--bv-falloff"}, true},
            {"min_reads_cluster", {"-r", "--min-reads-cluster"}, true}, {"repr_percentile", {"-p", "--repr-percentile"}, true},
            {"rna", {"--rna"}, false}, {"verbose", {"--verbose"}, false}, {"raw", {"--raw"}, false},
            {"lower_len", {"--lower-length"}, true}, {"upper_len", {"--upper-length"}, true}, {"device", {"--device"}, true},
            {"devices", {"--devices"}, true}, {"host-exchange", {"--host-exchange"}, false}, {"write-unzipped", {"--write-unzipped"}, false},
            {"count-pass", {"--count-pass"}, true}, {"report", {"--report"}, false}});
        const char *usage = "rattle cluster -i reads.fq [-o dir] [--rna] [--iso] ... (flags of RATTLE's cluster mode)\n"
                            "  --report           also write cluster_report.tsv: one line per join (a read joining a cluster's founder, or a cluster\n"
                            "                     joining another through their representatives) with the comparison that decided it: pass,\n"
                            "                     bit-vector threshold, strand, bases, hc_bases, min_len, score, variance (one device only)\n"
                            "  --devices 0,1,..   one job over several GPUs (RCCL; --host-exchange: in-process exchange on host buffers)\n"
                            "  --count-pass auto|seed|search|index   form of the count pass (what RATTLE_PAIR_COUNT sets; default auto)\n";
        if (a.has("count-pass")) {
            // the library reads the variable once, at its first evaluation: set it before any device thread starts
            const std::string form = a.str("count-pass", "auto");
            if (count_pass_of(form, usage) == 0) unsetenv("RATTLE_PAIR_COUNT");
            else setenv("RATTLE_PAIR_COUNT", form.c_str(), 1);
        }
        if (a.has("help")) {
            std::cerr << usage <<
                         "  --write-unzipped   also write the inflated copy of a .gz input next to it, as the reference does\n";
            exit(EXIT_SUCCESS);
        }
        if (!a.has("input")) die("ERROR: No input file provided");
        k = a.i("kmer_size", 10); iso_k = a.i("iso_kmer_size", 11);
        if (k > 16 || iso_k > 16) die("\nError: maximum kmer size = 16 \n");
        outdir = output_dir(a);
        is_rna = a.has("rna"); want_report = a.has("report");
        one_device_only(a, "report", "cluster report");
        std::cerr << "RNA mode: " << std::boolalpha << is_rna << std::endl;
    }
    // main.cpp:16-64 + fasta.cpp:272-370: ann = running record index over ALL records, length filter unless --raw, reads that
    // contain 'N' skipped; then sort_read_set (fasta.cpp:458-464): stable, longest first (a counting sort over the lengths)
    void filter_and_sort() {
        const bool raw = a.has("raw");
        const int lo = a.i("lower_len", 150), hi = a.i("upper_len", 100000);
        const size_t n = T.n();
        std::vector<uint8_t> keep(n, 0);
        std::atomic<size_t> n_skipped(0);
        parallel_chunks(n, [&](size_t b, size_t e) {
            size_t sk = 0;
            for (size_t i = b; i < e; ++i) {
                const span sq = T.seq[i];
                if (!(raw || ((int)sq.n >= lo && (int)sq.n <= hi))) continue;
                if (memchr(sq.p, 'N', sq.n)) { ++sk; continue; }
                keep[i] = 1;
            }
            n_skipped += sk;
        });
        if (n_skipped) std::cerr << "\n" << n_skipped << "  reads contains N are skipped!" << std::endl;
        uint32_t max_len = 0;
        for (size_t i = 0; i < n; ++i) if (keep[i]) max_len = std::max(max_len, T.seq[i].n);
        std::vector<uint32_t> start((size_t)max_len + 2, 0);
        for (size_t i = 0; i < n; ++i) if (keep[i]) ++start[max_len - T.seq[i].n + 1];
        for (size_t b = 0; b <= max_len; ++b) start[b + 1] += start[b];
        order.resize(start[(size_t)max_len + 1]);
        for (size_t i = 0; i < n; ++i) if (keep[i]) order[start[max_len - T.seq[i].n]++] = (uint32_t)i;
    }
    // the devices open on a helper thread while the input is read, filtered, sorted and gathered
    void read_input() {
        std::cerr << "Reading fasta file... " << std::endl;
        opener.start(team, a, 0);
        { cli_timer t("read input"); read_table_inputs(T, split_string(a.str("input", ""), ','), split_string(a.str("label", ""), ','), a.has("write-unzipped")); }
        {
            cli_timer t("filter + sort + gather");
            filter_and_sort();
            std::cout << "Reads: " << order.size() << std::endl;
            gather_reads(T, order, cat, nullptr, off);
            std::cerr << "Done" << std::endl;
        }
        cli_timer t("wait for device");
        opener.wait();
    }
    // cluster_report.tsv: one line per join, in the library's order; ids_of: the set's ids -> processing positions (null: identity)
    void report_rows(const rattle_cluster_set *cs, int level, const cseq_t *ids_of) {
        rattle_cluster_report *rp = nullptr;
        chk(rattle_hip_cluster_report(cs, &rp));
        auto name = [&](int32_t id) { return record_name(T.header[order[ids_of ? (uint32_t)ids_of[id].seq_id : (uint32_t)id]]); };
        for (uint64_t i = 0; i < rp->n; ++i)
            report_text += std::to_string(level) + "\t" + std::to_string(rp->pass[i]) + "\t" + g17(rp->bv_threshold[i]) + "\t" + name(rp->absorbed[i]) + "\t" +
                           name(rp->into[i]) + "\t" + (rp->rev[i] ? "-" : "+") + "\t" + std::to_string(rp->bases[i]) + "\t" +
                           std::to_string(rp->hc_bases[i]) + "\t" + std::to_string(rp->min_len[i]) + "\t" + g17(rp->score[i]) + "\t" + g17(rp->variance[i]) + "\n";
        rattle_hip_cluster_report_free(rp);
    }
    void gene_level() {
        rattle_cluster_set *raw = nullptr;
        {
            cli_timer t("library: load + cluster");
            P.t_s = a.d("t_s", P.t_s); P.t_v = a.d("t_v", P.t_v); P.bv_threshold = a.d("bv_threshold", P.bv_threshold);
            P.min_bv_threshold = a.d("bv_min_threshold", P.min_bv_threshold); P.bv_falloff = a.d("bv_falloff", P.bv_falloff);
            P.min_reads_cluster = a.i("min_reads_cluster", 0); P.repr_percentile = a.d("repr_percentile", P.repr_percentile);
            P.is_rna = is_rna ? 1 : 0;
            team.run([&](int r, rattle_ctx *ctx) {                                      // every rank ends up with the same clusters
                if (want_report) chk(rattle_hip_set_cluster_report(ctx, 1));
                chk(rattle_hip_load_reads(ctx, cat.data(), off.data(), (uint32_t)order.size(), k, is_rna ? 0 : 1));
                rattle_cluster_set *mine = nullptr;
                chk(rattle_hip_cluster_reads(ctx, &P, &mine));
                if (r == 0) raw = mine; else rattle_hip_cluster_set_free(mine);
            });
        }
        t_out.reset(new cli_timer("to clusters.out"));
        if (want_report) report_rows(raw, 0, nullptr);
        clusters = to_set(raw);
        std::cerr << "Gene clustering done" << std::endl;
        std::cerr << clusters.size() << " gene clusters found" << std::endl;
    }
    // main.cpp:281-323: second level per gene cluster with the iso parameters.  All gene clusters at once: the subsets are
    // independent (rattle_hip_cluster_subsets runs them concurrently, and over the ranks when there are several)
    void iso_level() {
        P.t_s = a.d("iso_t_s", 0.3); P.t_v = a.d("iso_t_v", 25);
        cluster_set_t gene = std::move(clusters), iso;
        std::vector<uint32_t> ids;
        std::vector<uint64_t> sub_off(1, 0);
        for (auto &c : gene) {
            std::stable_sort(c.seqs.begin(), c.seqs.end(), [](const cseq_t &x, const cseq_t &y) { return x.seq_id > y.seq_id; });
            std::stable_sort(c.seqs.begin(), c.seqs.end(), [&](const cseq_t &x, const cseq_t &y) { return off[x.seq_id + 1] - off[x.seq_id] > off[y.seq_id + 1] - off[y.seq_id]; });
            for (auto &s : c.seqs) ids.push_back((uint32_t)s.seq_id);
            sub_off.push_back(ids.size());
        }
        std::vector<rattle_cluster_set *> subs(gene.size() ? gene.size() : 1, nullptr);
        team.run([&](int r, rattle_ctx *ctx) {
            chk(rattle_hip_load_reads(ctx, cat.data(), off.data(), (uint32_t)order.size(), iso_k, is_rna ? 0 : 1));
            std::vector<rattle_cluster_set *> mine(gene.size() ? gene.size() : 1, nullptr);
            chk(rattle_hip_cluster_subsets(ctx, &P, ids.data(), sub_off.data(), (uint32_t)gene.size(), mine.data(), 0));
            if (r == 0) subs = mine; else for (auto *x : mine) rattle_hip_cluster_set_free(x);
        });
        int gi = 0;
        for (auto &c : gene) {
            if (want_report) report_rows(subs[gi], 1, c.seqs.data());
            for (auto &ic : to_set(subs[gi])) {
                cluster_t o;
                o.main_seq = cseq_t{c.seqs[ic.main_seq.seq_id].seq_id, ic.main_seq.rev, gi};
                for (auto &s : ic.seqs) o.seqs.push_back(cseq_t{c.seqs[s.seq_id].seq_id, s.rev, gi});
                iso.push_back(o);
            }
            ++gi;
        }
        std::cerr << "Isoform clustering done" << std::endl;
        std::cerr << iso.size() << " isoform clusters found" << std::endl;
        clusters = std::move(iso);
    }
    void write() {                                                                   // clusters.out holds record indices (main.cpp:264-277)
        for (auto &c : clusters) {
            c.main_seq.seq_id = (int)order[c.main_seq.seq_id];
            for (auto &s : c.seqs) s.seq_id = (int)order[s.seq_id];
        }
        write_clusters(clusters, outdir + "/clusters.out");
        if (want_report) write_text(outdir + "/cluster_report.tsv", report_text);
        team.close();
        t_out.reset();
    }
};

int mode_cluster(int argc, char **argv) {
    cluster_job J;
    J.options(argc, argv);
    J.read_input();
    J.gene_level();
    if (J.a.has("iso")) J.iso_level();
    J.write();
    return EXIT_SUCCESS;
}

// ---- `rattle assign` -----------------------------------------------------------------------------------------------------
// The reads of -i placed on the transcripts of -x by their best cluster_together score (include/rattle_hip.h, "assign").
// Every record of both files takes part, in file order: there is no length filter and no sort.  A read with a base other than A, C,
// G, T, U is not compared and comes out unassigned (`cluster` skips such reads).  --paf: every placed read is then aligned to its transcript
// (include/rattle_hip.h, "align_pairs") and alignments.paf appears beside the two tables.  --secondary N: the N next-best transcripts of
// every read beside its best (include/rattle_hip.h, "The candidate list") as candidates.tsv, and with --paf each of them aligned.
// --abundance: the list is made with 8 slots, the EM of include/rattle_hip.h, "abundance", runs over it, and abundance.tsv appears; the
// other writers see the first --secondary + 1 slots, which are what the shorter list holds.
struct assign_job {
    args_t a;
    int k = 10;
    std::string outdir;
    rattle_assign_params P;
    device_team team;
    team_opener opener;                           // opens `team` behind the reading of the input
    read_table R, X;                              // the reads and the transcripts
    std::vector<uint32_t> rid, xid;               // the records that are submitted: the clean reads, every transcript
    byte_buf rcat, xcat;
    std::vector<uint64_t> roff, xoff;
    rattle_assignment *A = nullptr;
    uint32_t secondary = 0;                       // --secondary N: N + 1 candidates per read
    rattle_candidates *C = nullptr;
    bool want_paf = false, want_cigar = false;     // --paf, --cigar (cg:Z: on every PAF line)
    rattle_align_params AP;
    bool want_scoring = false;                    // --paf-scoring m,x,o,e: affine gaps, the three-state kernels
    rattle_align_scoring AS;
    bool want_ends = false;                       // --paf-end-to-end: the whole read on every line (RATTLE_ALIGN_READ)
    bool want_abundance = false;                  // --abundance: the candidate list with 8 slots, the EM over it, abundance.tsv
    rattle_abundance_params EP;
    rattle_abundance *E = nullptr;
    bool want_pileup = false;                     // --pileup: the alignment of every read on its transcript also fills kernel G's table
    rattle_pileup *U = nullptr;
    std::string text, counts, paf, cand, abund;   // assignments.tsv, target_counts.tsv, alignments.paf (--paf), candidates.tsv (--secondary), abundance.tsv (--abundance)
    std::string pile;                             // pileup.tsv (--pileup)
    void options(int argc, char **argv) {
        a = parse(argc, argv, {
            {"help", {"-h", "--help"}, false}, {"input", {"-i", "--input"}, true}, {"targets", {"-x", "--transcripts"}, true},
            {"output", {"-o", "--output"}, true}, {"kmer_size", {"-k", "--kmer-size"}, true}, {"t_s", {"-s", "--score-threshold"}, true},
            {"t_v", {"-v", "--max-variance"}, true}, {"bv_threshold", {"-B", "--bv-start-threshold"}, true}, {"rna", {"--rna"}, false},
            {"count-pass", {"--count-pass"}, true}, {"device", {"--device"}, true}, {"devices", {"--devices"}, true},
            {"target-batch", {"--target-batch"}, true}, {"read-chunk", {"--read-chunk"}, true}, {"paf", {"--paf"}, false},
            {"paf-max-cells", {"--paf-max-cells"}, true}, {"cigar", {"--cigar"}, false}, {"paf-scoring", {"--paf-scoring"}, true},
            {"secondary", {"--secondary"}, true}, {"paf-end-to-end", {"--paf-end-to-end"}, false}, {"abundance", {"--abundance"}, false},
            {"abundance-ratio", {"--abundance-ratio"}, true}, {"abundance-tol", {"--abundance-tol"}, true},
            {"abundance-iters", {"--abundance-iters"}, true}, {"pileup", {"--pileup"}, false}});
        const char *usage = "rattle assign -i reads.fq -x transcripts.fq [-o dir] [-k 10] [-s 0.2] [-v 1000000] [-B 0.4] [--rna] [--device n] [--paf [--cigar] [--pileup]] [--secondary n] [--abundance]\n"
                            "  places every read of -i on the transcript of -x that accepts it with the best score (the comparison `cluster` joins\n"
                            "  reads by, the transcript in the seed's role) and writes assignments.tsv (one line per read: target, strand, score,\n"
                            "  second_score, n_accepted, bases, hc_bases, min_len, variance) and target_counts.tsv (reads per transcript)\n"
                            "  --count-pass auto|seed|search|index   form of the count pass (default auto)\n"
                            "  --target-batch n / --read-chunk n     transcripts per evaluation / reads indexed at a time (the result does not depend on them)\n"
                            "  --paf                                 also align every placed read to its transcript (local, match 5, mismatch -4, gap -8 per\n"
                            "                                        column) and write alignments.paf: one PAF line per aligned read, in file order\n"
                            "  --paf-max-cells n                     with --paf: skip a read whose length x its transcript's length exceeds n (default 0: no limit)\n"
                            "  --cigar                               with --paf: end every line of alignments.paf with cg:Z:<CIGAR>, the alignment's columns\n"
                            "                                        in the extended set (= match, X mismatch, I read base on a gap, D transcript base on a gap)\n"
                            "  --paf-scoring m,x,o,e                 with --paf: affine gaps and this scoring, four positive integers: match +m, mismatch -x,\n"
                            "                                        the first column of a gap -o, every further one -e; each in 1..64, e <= o.  5,4,8,6 is the\n"
                            "                                        scoring of `correct`, 2,4,4,2 minimap2's.  Default: linear gaps, 5,4,8,8\n"
                            "  --paf-end-to-end                      with --paf: align every read from its first base to its last, the transcript's ends free\n"
                            "                                        (semi-global): nothing is clipped, an overhang or a foreign exon shows as I or X at the\n"
                            "                                        line's end, AS may be negative, and the AS of --secondary's ranks are comparable\n"
                            "  --pileup                              with --paf: also write pileup.tsv, one line per transcript position that a read covers:\n"
                            "                                        target, pos (0-based), ref, depth, A, C, G, T (the reads' bases there, on the transcript's\n"
                            "                                        strand), del, ins (insertions before this base), starts, ends (alignments that begin / end\n"
                            "                                        here).  Counted on the device from the alignments of alignments.paf (with --secondary: the\n"
                            "                                        tp:A:P lines); --cigar is not needed.  The other files do not change\n"
                            "  --secondary n                         n in 1..7: also write candidates.tsv, the best transcript of every read and its n next-best\n"
                            "                                        (one line per read and rank: read, rank, target, strand, score, bases, hc_bases, min_len,\n"
                            "                                        variance); with --paf every one of them is aligned, and each line of alignments.paf carries\n"
                            "                                        tp:A:P (rank 0) or tp:A:S and rk:i:<rank>.  The other two files do not change\n"
                            "  --abundance                           also write abundance.tsv, one line per transcript: target, length, reads, unique_reads,\n"
                            "                                        compatible_reads, est_reads, cpm.  est_reads shares every read among the transcripts that\n"
                            "                                        accept it nearly as well as its best one (an EM over its 8 best transcripts, on the device,\n"
                            "                                        in integer fixed point: the same bits on every run).  The other files do not change\n"
                            "  --abundance-ratio f                   with --abundance: a transcript is compatible with a read if its score reaches f times the\n"
                            "                                        read's best score; f in (0, 1] (default 0.95)\n"
                            "  --abundance-tol f                     with --abundance: stop when no estimate moved by more than f reads; 0 <= f < 2^20 (default 0.001)\n"
                            "  --abundance-iters n                   with --abundance: at most n iterations, n >= 1 (default 1000)\n";
        if (a.has("help")) { std::cerr << usage; exit(EXIT_SUCCESS); }
        if (!a.has("input")) die("ERROR: No input file provided (-i reads)");
        if (!a.has("targets")) die("ERROR: No transcript file provided (-x transcripts)");
        if (a.has("devices")) die("\nError: assign runs on one device: --devices is not available, use --device\n");
        memset(&P, 0, sizeof P);
        P.count_pass = count_pass_of(a.str("count-pass", "auto"), usage);
        k = a.i("kmer_size", 10);
        if (k > 16) die("\nError: maximum kmer size = 16 \n");
        outdir = output_dir(a);
        P.t_s = a.d("t_s", 0.2); P.t_v = a.d("t_v", 1000000); P.bv_threshold = a.d("bv_threshold", 0.4);
        P.is_rna = a.has("rna") ? 1 : 0;
        want_paf = a.has("paf");
        if (a.has("paf-max-cells") && !want_paf) die("\nError: --paf-max-cells needs --paf\n");
        want_cigar = a.has("cigar");
        if (want_cigar && !want_paf) die("\nError: --cigar needs --paf\n");
        want_scoring = a.has("paf-scoring");
        if (want_scoring && !want_paf) die("\nError: --paf-scoring needs --paf\n");
        if (want_scoring) {
            const char *limit = "\nError: --paf-scoring takes four integers m,x,o,e, each in 1..64 and e <= o (match, mismatch, gap open, gap extend)\n";
            const std::vector<std::string> v = split_string(a.str("paf-scoring", ""), ',');
            uint32_t w[4] = {0, 0, 0, 0};
            if (v.size() != 4) die(limit);
            for (int i = 0; i < 4; ++i) {
                if (v[i].empty() || v[i].size() > 2 || v[i].find_first_not_of("0123456789") != std::string::npos) die(limit);
                w[i] = (uint32_t)std::stoul(v[i]);
                if (w[i] < 1 || w[i] > 64) die(limit);
            }
            if (w[3] > w[2]) die(limit);
            AS.match = w[0]; AS.mismatch = w[1]; AS.gap_open = w[2]; AS.gap_extend = w[3];
        }
        want_ends = a.has("paf-end-to-end");
        if (want_ends && !want_paf) die("\nError: --paf-end-to-end needs --paf\n");
        want_pileup = a.has("pileup");
        if (want_pileup && !want_paf) die("\nError: --pileup needs --paf\n");
        if (a.has("secondary")) {
            const std::string v = a.str("secondary", "");
            if (v.size() != 1 || v[0] < '1' || v[0] > '7') die("\nError: --secondary takes a number of further transcripts per read in 1..7\n");
            secondary = (uint32_t)(v[0] - '0');
        }
        want_abundance = a.has("abundance");
        for (const char *f : {"abundance-ratio", "abundance-tol", "abundance-iters"})
            if (a.has(f) && !want_abundance) die(std::string("\nError: --") + f + " needs --abundance\n");
        EP.ratio = 0.95; EP.tol = 1e-3; EP.max_iters = 1000; EP.iter_block = 0;
        if (want_abundance) {
            // the number an option holds; NaN, which every limit below refuses, for anything else
            auto number = [&](const char *f, double fallback) {
                if (!a.has(f)) return fallback;
                const std::string v = a.str(f, "");
                char *end = nullptr;
                const double x = strtod(v.c_str(), &end);
                return (v.empty() || *end) ? std::nan("") : x;
            };
            EP.ratio = number("abundance-ratio", 0.95);
            if (!(EP.ratio > 0.0 && EP.ratio <= 1.0)) die("\nError: --abundance-ratio takes a number in (0, 1]\n");
            EP.tol = number("abundance-tol", 1e-3);
            if (!(EP.tol >= 0.0 && EP.tol < 1048576.0)) die("\nError: --abundance-tol takes a number of reads in [0, 2^20)\n");
            const double it = number("abundance-iters", 1000);
            if (!(it >= 1.0 && it <= 4294967295.0) || it != std::floor(it)) die("\nError: --abundance-iters takes a whole number of iterations, at least 1\n");
            EP.max_iters = (uint32_t)it;
        }
        memset(&AP, 0, sizeof AP);
        AP.max_cells = std::stoull(a.str("paf-max-cells", "0"));
        P.target_batch = (uint32_t)std::max(0, a.i("target-batch", 0)); P.read_chunk = (uint32_t)std::max(0, a.i("read-chunk", 0));
        std::cerr << "RNA mode: " << std::boolalpha << (P.is_rna != 0) << std::endl;
    }
    // both files, the alphabet screen and the gather, while the device opens
    void read_input() {
        opener.start(team, a, 0);
        { cli_timer t("read input"); read_table_inputs(R, split_string(a.str("input", ""), ','), {}, false); read_table_inputs(X, split_string(a.str("targets", ""), ','), {}, false); }
        auto clean = [](const span &s) { for (uint32_t i = 0; i < s.n; ++i) if (!strchr("ACGTU", s.p[i]) || !s.p[i]) return false; return true; };
        xid.resize(X.n());
        for (size_t i = 0; i < X.n(); ++i) {
            if (!clean(X.seq[i])) die("\nError: transcript " + X.head(i) + " has a base other than A, C, G, T, U\n");
            xid[i] = (uint32_t)i;
        }
        for (size_t i = 0; i < R.n(); ++i) if (clean(R.seq[i])) rid.push_back((uint32_t)i);
        if (rid.size() != R.n()) std::cerr << "\n" << R.n() - rid.size() << "  reads with a base other than A, C, G, T, U are left unassigned" << std::endl;
        std::cout << "Reads: " << R.n() << ", transcripts: " << X.n() << std::endl;
        gather_reads(R, rid, rcat, nullptr, roff);
        gather_reads(X, xid, xcat, nullptr, xoff);
        opener.wait();
    }
    void run() {
        cli_timer t("library: assign");
        if (secondary || want_abundance) chk(rattle_hip_assign_reads_top(team.ctx[0], xcat.data(), xoff.data(), (uint32_t)xid.size(), rcat.data(), roff.data(), (uint32_t)rid.size(), k, &P, want_abundance ? 8 : secondary + 1, &A, &C));
        else chk(rattle_hip_assign_reads(team.ctx[0], xcat.data(), xoff.data(), (uint32_t)xid.size(), rcat.data(), roff.data(), (uint32_t)rid.size(), k, &P, &A));
    }
    // --abundance: the EM over the 8-slot list of the submitted reads (the reads that were not submitted have no candidate)
    void estimate() {
        cli_timer t("library: abundance");
        chk(rattle_hip_abundance(team.ctx[0], C, (uint32_t)xid.size(), &EP, &E));
        uint64_t full = 0;
        for (uint32_t r = 0; r < C->n; ++r) full += C->count[r] == C->k;
        std::cerr << "abundance: " << E->iterations << " iterations" << (E->converged ? "" : ", not converged") << "; " << full << " reads fill all "
                  << C->k << " candidate slots (further transcripts may accept them)" << std::endl;
    }
    // the ranks the writers of --secondary see: the list holds 8 under --abundance, and its first ranks are what the shorter list holds
    uint32_t ranks() const { return std::min(C->k, secondary + 1); }
    // the submitted reads on target[r] / rev[r] each (-1: not aligned): one call of the library; with `table` (--pileup, the reads on
    // their own transcripts) the call that also counts, which returns the same records and, under --cigar, the same ops
    void align_on(const int32_t *target, const uint8_t *rev, rattle_alignment **L, rattle_cigars **G, rattle_pileup **table = nullptr) {
        const rattle_align_scoring *S = want_scoring ? &AS : nullptr;
        const int mode = want_ends ? RATTLE_ALIGN_READ : RATTLE_ALIGN_LOCAL;      // (local through the _mode calls is the plain call, name and all)
        const uint32_t nt = (uint32_t)xid.size(), nr = (uint32_t)rid.size();
        if (table) chk(rattle_hip_align_pileup(team.ctx[0], xcat.data(), xoff.data(), nt, rcat.data(), roff.data(), nr, target, rev, &AP, S, mode, L, want_cigar ? G : nullptr, table));
        else if (want_cigar) chk(rattle_hip_align_cigars_mode(team.ctx[0], xcat.data(), xoff.data(), nt, rcat.data(), roff.data(), nr, target, rev, &AP, S, mode, L, G));
        else chk(rattle_hip_align_pairs_mode(team.ctx[0], xcat.data(), xoff.data(), nt, rcat.data(), roff.data(), nr, target, rev, &AP, S, mode, L));
    }
    // the PAF line of submitted read `at` on transcript x; tags: what stands between nd:i: and cg:Z:
    void paf_line(uint32_t at, uint32_t x, bool rev, const rattle_alignment *L, const rattle_cigars *G, const std::string &tags) {
        const uint64_t gaps = (uint64_t)L->q_gap[at] + L->t_gap[at], cols = (uint64_t)L->matches[at] + L->mismatches[at] + gaps;
        paf += record_name(R.header[rid[at]]) + "\t" + std::to_string(R.seq[rid[at]].n) + "\t" + std::to_string(L->q_start[at]) + "\t" + std::to_string(L->q_end[at]) + "\t" +
               (rev ? "-" : "+") + "\t" + record_name(X.header[x]) + "\t" + std::to_string(X.seq[x].n) + "\t" + std::to_string(L->t_start[at]) + "\t" +
               std::to_string(L->t_end[at]) + "\t" + std::to_string(L->matches[at]) + "\t" + std::to_string(cols) + "\t255\tAS:i:" + std::to_string(L->score[at]) +
               "\tNM:i:" + std::to_string(L->mismatches[at] + gaps) + "\tnx:i:" + std::to_string(L->mismatches[at]) + "\tni:i:" + std::to_string(L->q_gap[at]) +
               "\tnd:i:" + std::to_string(L->t_gap[at]) + tags;
        if (G) {
            paf += "\tcg:Z:";
            for (uint64_t o = G->offset[at]; o < G->offset[at + 1]; ++o) {
                const uint32_t op = G->ops[o] & 15u;
                paf += std::to_string(G->ops[o] >> 4) + (op == 7 ? "=" : op == 8 ? "X" : op == 1 ? "I" : "D");
            }
        }
        paf += "\n";
    }
    // --paf: the submitted reads on the transcripts `run` placed them on; one PAF line per read that aligns, in file order
    void align() {
        cli_timer t(want_pileup ? "library: align_pileup" : want_cigar ? "library: align_cigars" : "library: align_pairs");
        rattle_alignment *L = nullptr;
        rattle_cigars *G = nullptr;
        align_on(A->target, A->rev, &L, &G, want_pileup ? &U : nullptr);
        uint64_t skipped = 0;
        for (uint32_t at = 0; at < L->n; ++at) {
            skipped += L->status[at] == 2;
            if (L->status[at] == 0) paf_line(at, (uint32_t)A->target[at], A->rev[at] != 0, L, G, "");
        }
        rattle_hip_alignment_free(L);
        rattle_hip_cigars_free(G);
        if (skipped) std::cerr << "\n" << skipped << "  reads over --paf-max-cells are left out of alignments.paf" << std::endl;
    }
    // --paf --secondary: one call per rank, every read on its slot of that rank, up to the first rank no read has; then one PAF line
    // per (read, rank) that aligns, in file order and then by rank
    void align_ranks() {
        cli_timer t(want_pileup ? (want_cigar ? "library: align_pileup (rank 0), align_cigars, every rank" : "library: align_pileup (rank 0), align_pairs, every rank")
                                : want_cigar ? "library: align_cigars, every rank" : "library: align_pairs, every rank");
        const uint32_t n = C->n, K = C->k;
        std::vector<rattle_alignment *> L;
        std::vector<rattle_cigars *> G;
        std::vector<int32_t> target(std::max<uint32_t>(1, n));
        std::vector<uint8_t> rev(std::max<uint32_t>(1, n));
        for (uint32_t j = 0; j < ranks(); ++j) {
            bool any = false;
            for (uint32_t r = 0; r < n; ++r) { target[r] = C->target[(size_t)r * K + j]; rev[r] = C->rev[(size_t)r * K + j]; any = any || C->count[r] > j; }
            if (!any) break;
            L.push_back(nullptr); G.push_back(nullptr);
            align_on(target.data(), rev.data(), &L.back(), &G.back(), want_pileup && j == 0 ? &U : nullptr);      // rank 0: the tp:A:P alignments
        }
        uint64_t skipped = 0;
        for (uint32_t at = 0; at < n; ++at)
            for (uint32_t j = 0; j < C->count[at] && j < L.size(); ++j) {                 // (L.size() <= ranks())
                skipped += L[j]->status[at] == 2;
                if (L[j]->status[at] != 0) continue;
                paf_line(at, (uint32_t)C->target[(size_t)at * K + j], C->rev[(size_t)at * K + j] != 0, L[j], G[j],
                         std::string(j == 0 ? "\ttp:A:P" : "\ttp:A:S") + "\trk:i:" + std::to_string(j));
            }
        for (size_t j = 0; j < L.size(); ++j) { rattle_hip_alignment_free(L[j]); rattle_hip_cigars_free(G[j]); }
        if (skipped) std::cerr << "\n" << skipped << "  pairs over --paf-max-cells are left out of alignments.paf" << std::endl;
    }
    // --pileup: one line per transcript position a read covers, in file order (no table: nothing was aligned)
    void format_pileup() {
        pile = "target\tpos\tref\tdepth\tA\tC\tG\tT\tdel\tins\tstarts\tends\n";
        uint64_t covered = 0, deepest = 0;
        for (size_t x = 0; U && x < xid.size(); ++x) {
            const std::string name = record_name(X.header[xid[x]]);
            for (uint64_t p = xoff[x]; p < xoff[x + 1] && p < U->n; ++p) {
                const uint64_t depth = (uint64_t)U->a[p] + U->c[p] + U->g[p] + U->t[p] + U->del[p];
                if (!depth) continue;
                ++covered; deepest = std::max(deepest, depth);
                pile += name + "\t" + std::to_string(p - xoff[x]) + "\t" + std::string(1, (char)xcat.data()[p]) + "\t" + std::to_string(depth) + "\t" + std::to_string(U->a[p]) + "\t" +
                        std::to_string(U->c[p]) + "\t" + std::to_string(U->g[p]) + "\t" + std::to_string(U->t[p]) + "\t" + std::to_string(U->del[p]) + "\t" +
                        std::to_string(U->ins[p]) + "\t" + std::to_string(U->starts[p]) + "\t" + std::to_string(U->ends[p]) + "\n";
            }
        }
        rattle_hip_pileup_free(U);
        std::cerr << "pileup: " << covered << " transcript positions covered, largest depth " << deepest << std::endl;
    }
    // --secondary: one line per filled slot, in file order of the reads, then by rank
    void format_candidates() {
        cand = "read\trank\ttarget\tstrand\tscore\tbases\thc_bases\tmin_len\tvariance\n";
        for (uint32_t at = 0; at < C->n; ++at)
            for (uint32_t j = 0; j < C->count[at] && j < ranks(); ++j) {
                const size_t s = (size_t)at * C->k + j;
                cand += record_name(R.header[rid[at]]) + "\t" + std::to_string(j) + "\t" + record_name(X.header[C->target[s]]) + "\t" + (C->rev[s] ? "-" : "+") + "\t" +
                        g17(C->score[s]) + "\t" + std::to_string(C->bases[s]) + "\t" + std::to_string(C->hc_bases[s]) + "\t" + std::to_string(C->min_len[s]) + "\t" +
                        g17(C->variance[s]) + "\n";
            }
    }
    // one line per read of -i, the reads that were not submitted included; then one line per transcript
    void format() {
        std::vector<uint64_t> n_best(X.n(), 0), n_unique(X.n(), 0);
        text = "read\ttarget\tstrand\tscore\tsecond_score\tn_accepted\tbases\thc_bases\tmin_len\tvariance\n";
        size_t at = 0;                                                                // next submitted read
        for (size_t i = 0; i < R.n(); ++i) {
            const bool sent = at < rid.size() && rid[at] == i;
            const int32_t t = sent ? A->target[at] : -1;
            text += record_name(R.header[i]) + "\t" + (t >= 0 ? record_name(X.header[t]) : std::string("*")) + "\t" + (t < 0 ? "*" : A->rev[at] ? "-" : "+") + "\t" +
                    g17(sent ? A->score[at] : -1.0) + "\t" + g17(sent ? A->second_score[at] : -1.0) + "\t" + std::to_string(sent ? A->n_accepted[at] : 0u) + "\t" +
                    std::to_string(sent ? A->bases[at] : 0) + "\t" + std::to_string(sent ? A->hc_bases[at] : 0) + "\t" + std::to_string(sent ? A->min_len[at] : 0u) + "\t" +
                    g17(sent ? A->variance[at] : 0.0) + "\n";
            if (t >= 0) { ++n_best[t]; if (A->second_score[at] < 0) ++n_unique[t]; }
            if (sent) ++at;
        }
        rattle_hip_assignment_free(A);
        rattle_hip_candidates_free(C);
        counts = "target\tlength\treads\tunique_reads\n";
        for (size_t t = 0; t < X.n(); ++t)
            counts += record_name(X.header[t]) + "\t" + std::to_string(X.seq[t].n) + "\t" + std::to_string(n_best[t]) + "\t" + std::to_string(n_unique[t]) + "\n";
        if (!want_abundance) return;
        abund = "target\tlength\treads\tunique_reads\tcompatible_reads\test_reads\tcpm\n";
        for (size_t t = 0; t < X.n(); ++t)
            abund += record_name(X.header[t]) + "\t" + std::to_string(X.seq[t].n) + "\t" + std::to_string(n_best[t]) + "\t" + std::to_string(n_unique[t]) + "\t" +
                     std::to_string(E->compatible_reads[t]) + "\t" + g17(E->est_reads[t]) + "\t" + g17(E->cpm[t]) + "\n";
        rattle_hip_abundance_free(E);
    }
    void write() {
        write_text(outdir + "/assignments.tsv", text);
        write_text(outdir + "/target_counts.tsv", counts);
        if (want_paf) write_text(outdir + "/alignments.paf", paf);
        if (secondary) write_text(outdir + "/candidates.tsv", cand);
        if (want_abundance) write_text(outdir + "/abundance.tsv", abund);
        if (want_pileup) write_text(outdir + "/pileup.tsv", pile);
        team.close();
        std::cerr << "Done" << std::endl;
    }
};

int mode_assign(int argc, char **argv) {
    assign_job J;
    J.options(argc, argv);
    J.read_input();
    J.run();
    if (J.want_abundance) J.estimate();
    if (J.want_paf) { if (J.secondary) J.align_ranks(); else J.align(); }
    if (J.want_pileup) J.format_pileup();
    if (J.secondary) J.format_candidates();
    J.format();
    J.write();
    return EXIT_SUCCESS;
}

// ---- `rattle correct` ----------------------------------------------------------------------------------------------------
struct correct_job {
    args_t a;
    bool want_report = false, want_support = false, gene_mode = true;
    std::vector<std::string> labels, files;
    std::string outdir, corrected_path, corrected_tmp;
    device_team team;
    team_opener opener;                           // opens `team` behind the reading of the input
    read_table T;
    cluster_set_t clusters;
    byte_buf cat, qcat;                           // bases and qualities of every record, in file order, and their offsets
    std::vector<uint64_t> off;
    std::vector<uint32_t> coff;                   // the clusters' members, flattened
    std::vector<int32_t> mid;
    std::vector<uint8_t> mrev;
    rattle_correct_params P = default_correct_params();
    std::atomic<bool> early_done{false}, early_failed{false};   // corrected.fq.tmp, written from the library's callback
    rattle_correction *R = nullptr;
    read_set_t consensi;
    std::unique_ptr<cli_timer> t_out;
    void options(int argc, char **argv) {
        a = parse(argc, argv, {
            {"help", {"-h", "--help"}, false}, {"input", {"-i", "--input"}, true}, {"label", {"-l", "--label"}, true},
            {"clusters", {"-c", "--clusters"}, true}, {"output", {"-o", "--output"}, true}, {"gap-occ", {"-g", "--gap-occ"}, true},
            {"min-occ", {"-m", "--min-occ"}, true}, {"split", {"-s", "--split"}, true}, {"min-reads", {"-r", "--min-reads"}, true},
            {"threads", {"-t", "--threads"}, true}, {"verbose", {"--verbose"}, false}, {"device", {"--device"}, true},
            {"vote-order", {"--vote-order"}, true}, {"max-pack-cells", {"--max-pack-cells"}, true}, {"devices", {"--devices"}, true},
            {"host-exchange", {"--host-exchange"}, false}, {"write-unzipped", {"--write-unzipped"}, false}, {"report", {"--report"}, false},
            {"support", {"--support"}, false}});
        if (a.has("help")) {
            std::cerr << "rattle correct -i reads.fq -c clusters.out [-o dir] ... (flags of RATTLE's correct mode)\n"
                         "  --report             also write correction_report.tsv: per record of corrected.fq its lengths before and after, the bases\n"
                         "                       trimmed at either end, and how many columns matched, were substituted, kept against the\n"
                         "                       winner, inserted, deleted or kept against a gap winner\n"
                         "  --support            also write consensus_support.tsv: per record of consensi.fq how many reads stand behind every\n"
                         "                       base (support: reads that voted for it, depth: reads that voted in its column, composed through\n"
                         "                       the pack consensi for a cluster of several packs), the smallest ratio and the number of bases\n"
                         "                       with no majority; one device only.  consensi.fq itself keeps its qualities\n"
                         "  --max-pack-cells N   leave packs whose largest alignment needs more than N DP cells uncorrected (default: only\n"
                         "                       packs that do not fit the device are skipped); skipped packs are listed in skipped_packs.tsv\n"
                         "  --devices 0,1,..     one job over several GPUs (RCCL; --host-exchange: in-process exchange on host buffers)\n";
            exit(EXIT_SUCCESS);
        }
        if (!a.has("input")) die("ERROR: No input file provided");
        if (!a.has("clusters")) die("ERROR: No clusters file provided");
        want_report = a.has("report"); want_support = a.has("support");
        one_device_only(a, "support", "consensus support");
        labels = split_string(a.str("label", ""), ','); files = split_string(a.str("input", ""), ',');
        outdir = a.str("output", ".");
        corrected_path = outdir + "/corrected.fq"; corrected_tmp = corrected_path + ".tmp";
    }
    // the reads, the clusters and the gather, while the devices open and reserve their arenas
    void read_input() {
        std::cerr << "Reading fasta file... ";
        // arena hint: ~440 kB of FASTQ per pack of 200 one-kb reads, at most a device full of resident packs in each of two
        // column classes (1792 places x 18.4 MB + 2048 x 34.5 MB = 104 GB at 1e6 one-kb reads, round 4; a hint that falls short
        // costs a second allocation -- 2.7 s in the first end-to-end run of round 4, when the hint was 89 GB -- not the result).  The
        // driver clears what it hands out at ~20 ms per GB, so a generous hint is seconds of start-up.
        const uint64_t packs_hint = std::min<uint64_t>(input_bytes(files) / 440000 + 1, 3840);
        opener.start(team, a, packs_hint * (30ull << 20));
        { cli_timer t("read input"); read_table_inputs(T, files, labels, a.has("write-unzipped")); }
        std::cerr << "Done" << std::endl;
        {
            cli_timer t("read clusters + gather");
            clusters = read_clusters(a.str("clusters", ""));
            if (clusters.empty()) die("\nError: empty clusters file\n");
            gene_mode = clusters[0].main_seq.gene_id == -1;                          // correct.cpp:322
            std::vector<uint32_t> all(T.n());
            for (uint32_t i = 0; i < all.size(); ++i) all[i] = i;
            gather_reads(T, all, cat, &qcat, off);
            flatten_members(clusters, coff, mid, mrev);
            P.min_occ = a.d("min-occ", P.min_occ); P.gap_occ = a.d("gap-occ", P.gap_occ);
            P.split = a.i("split", P.split); P.min_reads = a.i("min-reads", P.min_reads);
            const std::string vo = a.str("vote-order", "");
            if (vo.size() == 6) memcpy(P.vote_order, vo.data(), 6);
            if (a.has("max-pack-cells")) P.max_pack_cells = std::stoull(a.str("max-pack-cells", "0"));
        }
        cli_timer t("wait for device + arena");
        opener.wait();
    }
    std::string tag(int cid) const {                                                 // correct.cpp:348-353
        const int gid = clusters[cid].main_seq.gene_id;
        if (gid == -1) return ",gene_cluster_" + std::to_string(cid);
        return ",gene_cluster_" + std::to_string(gid) + ",transcript_cluster_" + std::to_string(cid);
    }
    // corrected.fq / uncorrected.fq (fasta.cpp:436-445 record layout) straight from the library's buffers: the text of each
    // file is laid out by record offsets and filled in parallel
    bool write_set(const rattle_read_set &S, bool corrected, const std::string &path) const {
        std::vector<std::string> tags(clusters.size());
        std::vector<uint64_t> at((size_t)S.n + 1, 0);
        for (uint32_t i = 0; i < S.n; ++i) {
            const uint32_t rid = (uint32_t)S.read_id[i];
            std::string &tg = tags[S.cluster_id[i]];
            if (tg.empty()) tg = tag(S.cluster_id[i]);
            const uint64_t len = S.off[i + 1] - S.off[i];
            at[i + 1] = at[i] + T.header[rid].n + (T.label[rid] ? T.labels[T.label[rid] - 1].size() : 0) + tg.size() + 1 + len + 1 +
                        (corrected ? 1 : T.ann[rid].n) + 1 + len + 1;
        }
        sized_output text(path, at[S.n]);
        parallel_chunks(S.n, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; ++i) {
                const uint32_t rid = (uint32_t)S.read_id[i];
                char *o = text.p + at[i];
                auto put = [&o](const char *p, size_t n) { memcpy(o, p, n); o += n; };
                put(T.header[rid].p, T.header[rid].n);
                if (T.label[rid]) put(T.labels[T.label[rid] - 1].data(), T.labels[T.label[rid] - 1].size());
                put(tags[S.cluster_id[i]].data(), tags[S.cluster_id[i]].size()); *o++ = '\n';
                put(S.seq + S.off[i], S.off[i + 1] - S.off[i]); *o++ = '\n';
                if (corrected) *o++ = '+'; else put(T.ann[rid].p, T.ann[rid].n);
                *o++ = '\n';
                put(S.qual + S.off[i], S.off[i + 1] - S.off[i]); *o++ = '\n';
            }
        });
        return text.finish();
    }
    // rattle_correct_params::corrected_ready.  It runs on a library thread with kernels in flight, so it never exits the process: it
    // writes corrected.fq.tmp and records the outcome
    static void corrected_ready(void *user, const rattle_read_set_s *S, const uint32_t *) {
        correct_job *J = (correct_job *)user;
        cli_timer t("corrected.fq (behind the consensus stages)");
        if (J->write_set(*S, true, J->corrected_tmp)) J->early_done = true; else J->early_failed = true;
    }
    // corrected.fq is formatted and written from the library's corrected_ready callback, while POA #2 / #3 still run on the
    // device (one device: the sharded job reassembles its reads at the end).  The main thread renames corrected.fq.tmp once
    // correct_reads has returned 0 (the reference writes its three files only after correct_reads, main.cpp:405-411: a failed run
    // must not leave a complete-looking corrected.fq) or removes it and reports the failure.
    void run_library() {
        cli_timer t("library: correct_reads");
        if (team.n() == 1) { P.corrected_ready = corrected_ready; P.corrected_ready_user = this; }
        team.run([&](int r, rattle_ctx *ctx) {                                      // packs sharded over the ranks, result reassembled on rank 0
            rattle_correction *mine = nullptr, *merged = nullptr;
            if (want_report) chk(rattle_hip_set_correction_report(ctx, 1));
            if (want_support) chk(rattle_hip_set_consensus_support(ctx, 1));
            const int rc = rattle_hip_correct_reads(ctx, cat.data(), qcat.data(), off.data(), (uint32_t)T.n(), (uint32_t)clusters.size(), coff.data(), mid.data(),
                                                    mrev.data(), &P, &mine);
            if (rc != 0 && team.n() == 1) unlink(corrected_tmp.c_str());           // no half of a result stays behind
            chk(rc);
            if (team.n() == 1) { R = mine; return; }
            chk(rattle_hip_correction_gather(ctx, mine, 0, &merged));
            rattle_hip_correction_free(mine);
            if (r == 0) R = merged;
        });
        if (early_failed) { unlink(corrected_tmp.c_str()); die("Error: cannot write " + corrected_path); }
        if (early_done && rename(corrected_tmp.c_str(), corrected_path.c_str()) != 0) die("Error: cannot write " + corrected_path);
    }
    // correct.cpp:453-469: per cluster, how many reads of its packs carry each label.  Only packs that produced a pack consensus
    // count (as `reads=` does): packs the library skipped (budget rule: listed by their index among ALL packs of the cluster;
    // POA #1 / #2 beyond the device: by their index among the QUEUED packs) do not
    std::vector<std::vector<int>> count_labels() const {
        std::vector<std::vector<int>> counts(clusters.size(), std::vector<int>(labels.size(), 0));
        if (labels.empty()) return counts;
        std::set<std::pair<int, uint32_t>> skip_all, skip_queued;
        for (uint32_t i = 0; i < R->skipped.n; ++i) {
            if (R->skipped.stage[i] == 0) skip_all.insert({R->skipped.cluster_id[i], R->skipped.pack[i]});
            else if (R->skipped.stage[i] <= 2) skip_queued.insert({R->skipped.cluster_id[i], R->skipped.pack[i]});
        }
        for (size_t c = 0; c < clusters.size(); ++c) {
            int n = (int)clusters[c].seqs.size();
            if (n == 0) continue;
            int n_files = (n - 1) / P.split + 1;
            uint32_t queued = 0;
            for (int nf = 0; nf < n_files; ++nf) {
                int sz = (n - 1 - nf) / n_files + 1;
                if (sz <= P.min_reads) continue;
                if (skip_all.count({(int)c, (uint32_t)nf})) continue;
                if (skip_queued.count({(int)c, queued++})) continue;
                for (int j = nf; j < n; j += n_files) {
                    const std::string h = T.head(clusters[c].seqs[j].seq_id);
                    size_t p = h.find_first_of(",");
                    std::string rest = p == std::string::npos ? "" : h.substr(p + 1);
                    std::string lab = rest.substr(0, rest.find_first_of(","));
                    for (size_t l = 0; l < labels.size(); ++l) if (labels[l] == lab) counts[c][l]++;
                }
            }
        }
        return counts;
    }
    void consensus_headers() {                                                       // correct.cpp:495-549
        t_out.reset(new cli_timer("format + write outputs"));
        const std::vector<std::vector<int>> label_counts = count_labels();
        for (uint32_t i = 0; i < R->consensi.n; ++i) {
            const int cid = R->consensi.cluster_id[i];
            std::string lr;
            for (size_t l = 0; l < labels.size(); ++l) lr += labels[l] + ":" + std::to_string(label_counts[cid][l]) + ",";
            const std::string name = gene_mode ? "@gene_cluster_" + std::to_string(cid)
                                               : "@transcript_cluster_" + std::to_string(cid) + " gene_cluster_" + std::to_string(clusters[cid].main_seq.gene_id);
            consensi.push_back(consensus_record(R->consensi, i, name + " reads=" + std::to_string(R->consensi.n_reads[i]) + " labels=" + lr));
        }
    }
    // correction_report.tsv: one line per record of corrected.fq, in that file's order
    std::string correction_report_text() const {
        rattle_correction_report *rp = nullptr;
        chk(rattle_hip_correction_report(R, &rp));
        std::string text = "read\tcluster\tin_len\tout_len\ttrim_front\ttrim_back\tmatch\tsubstituted\tmismatch_kept\tinserted\tdeleted\tgap_kept\n";
        for (uint32_t i = 0; i < rp->n; ++i) {
            text += record_name(T.header[(uint32_t)R->corrected.read_id[i]]) + "\t" + std::to_string(R->corrected.cluster_id[i]);
            for (const uint32_t *v : {rp->in_len, rp->out_len, rp->trim_front, rp->trim_back, rp->match, rp->substituted, rp->mismatch_kept, rp->inserted,
                                      rp->deleted, rp->gap_kept})
                text += "\t" + std::to_string(v[i]);
            text += "\n";
        }
        rattle_hip_correction_report_free(rp);
        return text;
    }
    // consensus_support.tsv: one line per record of consensi.fq, in that file's order
    std::string consensus_support_text() const {
        rattle_consensus_support *sp = nullptr;
        chk(rattle_hip_consensus_support(R, &sp));
        std::string text = "consensus\tlength\tlevel\treads\tmin_ratio\tweak\tsupport\tdepth\n";
        for (uint32_t i = 0; i < sp->n; ++i) {
            const uint64_t p0 = sp->off[i], p1 = sp->off[i + 1];
            double min_ratio = 0.0;
            uint64_t weak = 0;
            for (uint64_t p = p0; p < p1; ++p) {
                const double ratio = double(sp->support[p]) / double(sp->depth[p]);
                if (p == p0 || ratio < min_ratio) min_ratio = ratio;
                weak += 2ull * sp->support[p] <= sp->depth[p];
            }
            text += record_name(consensi[i].header) + "\t" + std::to_string(p1 - p0) + "\t" + std::to_string((int)sp->level[i]) + "\t" +
                    std::to_string(R->consensi.n_reads[i]) + "\t" + g17(min_ratio) + "\t" + std::to_string(weak);
            for (const uint32_t *v : {sp->support, sp->depth}) {
                text += "\t";
                for (uint64_t p = p0; p < p1; ++p) { if (p > p0) text += ","; text += std::to_string(v[p]); }
            }
            text += "\n";
        }
        rattle_hip_consensus_support_free(sp);
        return text;
    }
    // skipped_packs.tsv: packs whose POA did not fit the device (or the --max-pack-cells budget): their reads are in uncorrected.fq
    std::string skipped_packs_text() const {
        std::string text = "cluster\tpack\tstage\treads\n";
        for (uint32_t i = 0; i < R->skipped.n; ++i)
            text += std::to_string(R->skipped.cluster_id[i]) + "\t" + std::to_string(R->skipped.pack[i]) + "\t" + std::to_string(R->skipped.stage[i]) + "\t" +
                    std::to_string(R->skipped.read_off[i + 1] - R->skipped.read_off[i]) + "\n";
        return text;
    }
    void write_outputs() {
        std::cerr << std::endl << "Generating consensi..." << std::endl;
        if (!early_done && !write_set(R->corrected, true, corrected_path)) die("Error: cannot write " + corrected_path);
        if (!write_set(R->uncorrected, false, outdir + "/uncorrected.fq")) die("Error: cannot write " + outdir + "/uncorrected.fq");
        write_fastq_file(consensi, outdir + "/consensi.fq");
        if (want_report) write_text(outdir + "/correction_report.tsv", correction_report_text());
        if (want_support) write_text(outdir + "/consensus_support.tsv", consensus_support_text());
        if (R->skipped.n) {
            write_text(outdir + "/skipped_packs.tsv", skipped_packs_text());
            std::cerr << R->skipped.n << " pack(s) with " << R->counters[4] << " reads were not corrected (DP beyond the device or the budget): skipped_packs.tsv" << std::endl;
        }
        t_out.reset();
        std::cerr << "Done" << std::endl;
        rattle_hip_correction_free(R);
        team.close();
    }
};

int mode_correct(int argc, char **argv) {
    correct_job J;
    J.options(argc, argv);
    J.read_input();
    J.run_library();
    J.consensus_headers();
    J.write_outputs();
    return EXIT_SUCCESS;
}

std::string reverse_complement(const std::string &seq) {          // utils.cpp:15-24
    std::string r(seq.size(), 'A');
    for (size_t i = 0; i < seq.size(); ++i) {
        char c = seq[seq.size() - 1 - i];
        r[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'T' ? 'A' : c == 'G' ? 'C' : c == 'U' ? 'A' : c;
    }
    return r;
}

// `rattle cluster_summary`, /root/reference/main.cpp:413-483 (host only, no device)
int mode_cluster_summary(int argc, char **argv) {
    std::vector<opt_def> defs = {{"help", {"-h", "--help"}, false}, {"input", {"-i", "--input"}, true}, {"label", {"-l", "--label"}, true},
                                 {"clusters", {"-c", "--clusters"}, true}};
    args_t a = parse(argc, argv, defs);
    if (a.has("help")) { std::cerr << "rattle cluster_summary -i reads.fq -c clusters.out\n"; return EXIT_SUCCESS; }
    if (!a.has("input")) die("ERROR: No input file provided");
    if (!a.has("clusters")) die("ERROR: No clusters file provided");
    std::cerr << "Reading fasta file... ";
    read_set_t reads = read_inputs(split_string(a.str("input", ""), ','), split_string(a.str("label", ""), ','));
    std::cerr << "Done" << std::endl;
    cluster_set_t clusters = read_clusters(a.str("clusters", ""));
    int cid = 0;
    for (auto &c : clusters) {
        for (auto &s : c.seqs) {
            if ((size_t)s.seq_id >= reads.size()) die("\nError: cluster member id out of range\n");
            if (c.main_seq.gene_id == -1) std::cout << reads[s.seq_id].header << ",gene_cluster_" << cid << "\n";
            else std::cout << reads[s.seq_id].header << ",gene_cluster_" << s.gene_id << ",transcript_cluster_" << cid << "\n";
        }
        ++cid;
    }
    return EXIT_SUCCESS;
}

// `rattle extract_clusters`, /root/reference/main.cpp:484-611 (host only, no device)
int mode_extract_clusters(int argc, char **argv) {
    std::vector<opt_def> defs = {{"help", {"-h", "--help"}, false}, {"input", {"-i", "--input"}, true}, {"label", {"-l", "--label"}, true},
                                 {"clusters", {"-c", "--clusters"}, true}, {"output", {"-o", "--output-folder"}, true},
                                 {"minreads", {"-m", "--min-reads"}, true}, {"fastq", {"--fastq"}, false}};
    args_t a = parse(argc, argv, defs);
    if (a.has("help")) { std::cerr << "rattle extract_clusters -i reads.fq -c clusters.out [-o dir] [-m N] [--fastq]\n"; return EXIT_SUCCESS; }
    if (!a.has("input")) die("ERROR: No input file provided");
    if (!a.has("clusters")) die("ERROR: No clusters file provided");
    if (a.has("output") && access(a.str("output", ".").c_str(), F_OK)) die("\nOutput folder doesn't exit. Please create it first. \n");
    std::cerr << "Reading fasta file... ";
    read_set_t reads = read_inputs(split_string(a.str("input", ""), ','), split_string(a.str("label", ""), ','));
    std::cerr << "Done" << std::endl;
    cluster_set_t clusters = read_clusters(a.str("clusters", ""));
    const int min_reads = a.i("minreads", 0);
    const bool fastq = a.has("fastq");
    int cid = 0;
    for (auto &c : clusters) {
        if ((int)c.seqs.size() > min_reads) {
            std::string fn = (a.has("output") ? a.str("output", ".") + "/" : std::string()) + "cluster_" + std::to_string(cid) + (fastq ? ".fq" : ".fa");
            std::ofstream f(fn);
            for (auto &s : c.seqs) {
                if ((size_t)s.seq_id >= reads.size()) die("\nError: cluster member id out of range\n");
                const read_t &r = reads[s.seq_id];
                if (c.main_seq.gene_id == -1) f << r.header << "\n";
                else f << r.header << "," << s.gene_id << "\n";
                f << (s.rev ? reverse_complement(r.seq) : r.seq) << "\n";          // quality is NOT reversed (main.cpp:585-588)
                if (fastq) f << r.ann << "\n" << r.quality << "\n";
            }
        }
        ++cid;
    }
    return EXIT_SUCCESS;
}

// ---- `rattle polish`, main.cpp:612-762 ----------------------------------------------------------------------------------------
// Cluster the consensi (k=6, 0.5, 25, bv 0.4/0.4 so no merge pass), correct with min_reads=0, rewrite the consensus headers.
struct polish_job {
    args_t a;
    bool is_rna = false, summary = false;
    std::vector<std::string> labels;
    read_set_t reads, out;                        // the input consensi, longest first; the records of transcriptome.fq
    std::string cat, qcat;                        // their bases and qualities (padded with '!' / cut to the sequence length)
    std::vector<uint64_t> off{0};
    rattle_ctx *ctx = nullptr;
    cluster_set_t clusters;
    rattle_correction *R = nullptr;
    std::string summary_text;                     // polish_summary.tsv: one line per input consensus
    void options(int argc, char **argv) {
        a = parse(argc, argv, {
            {"help", {"-h", "--help"}, false}, {"input", {"-i", "--input"}, true}, {"output", {"-o", "--output-folder"}, true},
            {"label", {"-l", "--label"}, true}, {"threads", {"-t", "--threads"}, true}, {"rna", {"--rna"}, false},
            {"verbose", {"--verbose"}, false}, {"summary", {"--summary"}, false}, {"device", {"--device"}, true}});
        if (a.has("help")) { std::cerr << "rattle polish -i consensi.fq [-o dir] [--rna] [--summary]\n"; exit(EXIT_SUCCESS); }
        if (!a.has("input")) die("ERROR: No input file provided");
        is_rna = a.has("rna"); summary = a.has("summary");
        labels = split_string(a.str("label", ""), ',');
    }
    void read_input() {
        std::cerr << "Reading fasta file... ";
        const std::string in = a.str("input", "");
        if (access(in.c_str(), F_OK)) die("\nError: Input file not found! \n");
        for_each_fastq_record(in, [&](const std::string &h, const std::string &s, const std::string &an, const std::string &q) {
            reads.push_back(read_t{h, s, an, q});
        });
        std::stable_sort(reads.begin(), reads.end(), [](const read_t &x, const read_t &y) { return x.seq.size() > y.seq.size(); });
        for (auto &r : reads) {
            cat += r.seq;
            std::string q = r.quality; q.resize(r.seq.size(), '!'); qcat += q;
            off.push_back(cat.size());
        }
        std::cerr << "Done" << std::endl;
    }
    void cluster() {
        std::cerr << "Clustering consensus sequences..." << std::endl;
        chk(rattle_hip_ctx_create(a.i("device", 0), &ctx));
        rattle_cluster_params P = default_cluster_params();
        P.t_s = 0.5; P.t_v = 25; P.min_bv_threshold = 0.4; P.is_rna = is_rna ? 1 : 0;
        chk(rattle_hip_load_reads(ctx, (const uint8_t *)cat.data(), off.data(), (uint32_t)reads.size(), 6, is_rna ? 0 : 1));
        rattle_cluster_set *raw = nullptr;
        chk(rattle_hip_cluster_reads(ctx, &P, &raw));
        clusters = to_set(raw);
    }
    void correct() {
        std::vector<uint32_t> coff;
        std::vector<int32_t> mid;
        std::vector<uint8_t> mrev;
        flatten_members(clusters, coff, mid, mrev);
        rattle_correct_params P = default_correct_params();
        P.min_reads = 0;
        chk(rattle_hip_correct_reads(ctx, (const uint8_t *)cat.data(), (const uint8_t *)qcat.data(), off.data(), (uint32_t)reads.size(),
                                     (uint32_t)clusters.size(), coff.data(), mid.data(), mrev.data(), &P, &R));
    }
    // main.cpp:690-755: a new consensus sums `reads=` and the label counts of the inputs it was made from.  Made from transcript-level
    // inputs it is one itself, and its gene follows the reference's gene_map: a member whose gene cluster is new maps that gene cluster
    // to the gene the record has so far (its own, if it has none), a member whose gene cluster was met before gives the record the
    // gene it maps to
    void rewrite_headers() {
        std::map<int, int> gene_map;
        for (uint32_t i = 0; i < R->consensi.n; ++i) {
            const int cid = R->consensi.cluster_id[i];           // == i: every cluster has a pack with min_reads = 0
            int gid = -1, total_reads = 0;
            std::vector<int> label_counts(labels.size(), 0);
            for (auto &m : clusters[cid].seqs) {
                const std::string &h = reads[m.seq_id].header;
                total_reads += std::stoi(split_string(h, '=').at(1));
                for (size_t l = 0; l < labels.size(); ++l) {
                    size_t idx = h.find(labels[l]);
                    if (idx != std::string::npos) {
                        std::string sub = h.substr(idx + 1);
                        label_counts[l] += std::stoi(sub.substr(sub.find_first_of(":") + 1));
                    }
                }
                auto info_c = split_string(h, '_');
                if (h.find("transcript_cluster") != std::string::npos) {
                    const int id = std::stoi(info_c.at(4));
                    if (gene_map.find(id) == gene_map.end()) { if (gid == -1) gid = id; gene_map.insert({id, gid}); }
                    else gid = gene_map.find(id)->second;
                    if (summary) summary_text += "transcript_cluster_" + std::to_string(std::stoi(info_c.at(2))) + ", gene_cluster_" + std::to_string(id) +
                                                 ", new_cluster_" + std::to_string(cid) + "\n";
                } else if (summary) {
                    summary_text += "gene_cluster_" + std::to_string(std::stoi(info_c.at(2))) + ", new_cluster_" + std::to_string(cid) + "\n";
                }
            }
            const std::string rcount = std::to_string(R->consensi.n_reads[i]);       // the "reads=" field correct_reads writes (correct.cpp:542)
            std::string header = gid != -1 ? "@transcript_cluster_" + std::to_string(cid) + " gene_cluster_" + std::to_string(gid) + " generated_from_transcript_clusters=" + rcount
                                           : "@cluster_" + std::to_string(cid) + " generated_from_consensi_clusters=" + rcount;
            header += " total_reads=" + std::to_string(total_reads) + " labels=";
            for (size_t l = 0; l < labels.size(); ++l) header += labels[l] + ":" + std::to_string(label_counts[l]) + ",";
            out.push_back(consensus_record(R->consensi, i, header));
        }
    }
    void write() {
        const std::string outdir = a.str("output", ".");
        if (summary) write_text(outdir + "/polish_summary.tsv", summary_text);
        write_fastq_file(out, outdir + "/transcriptome.fq");
        rattle_hip_correction_free(R);
        rattle_hip_ctx_destroy(ctx);
        std::cerr << "Done" << std::endl;
    }
};

int mode_polish(int argc, char **argv) {
    polish_job J;
    J.options(argc, argv);
    J.read_input();
    J.cluster();
    J.correct();
    J.rewrite_headers();
    J.write();
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char **argv) {
    setenv("GPU_MAX_HW_QUEUES", "12", 0);      // before the HIP runtime starts: the POA column classes of a pass run concurrently, one hardware queue each (poa.hip)
    const char *mode = argc < 2 ? "" : argv[1];
    try {
        if (!strcmp(mode, "cluster")) return mode_cluster(argc, argv);
        if (!strcmp(mode, "correct")) return mode_correct(argc, argv);
        if (!strcmp(mode, "polish")) return mode_polish(argc, argv);
        if (!strcmp(mode, "assign")) return mode_assign(argc, argv);
        if (!strcmp(mode, "cluster_summary")) return mode_cluster_summary(argc, argv);
        if (!strcmp(mode, "extract_clusters")) return mode_extract_clusters(argc, argv);
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
    std::cout << "Run with mode: ./rattle <cluster|cluster_summary|extract_clusters|correct|polish|assign>" << std::endl;
    return EXIT_FAILURE;
}
