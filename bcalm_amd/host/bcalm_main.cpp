// bcalm -- command-line host of the MI355X-native constructor.
//
// Keeps the reference's CLI surface and output contract, re-stated from scratch:
//   ./bcalm -in reads.fa -kmer-size 31 -abundance-min 2 [-out prefix] [-minimizer-size m]
//     /root/reference/README.md:11-25 (usage), src/bcalm_1.cpp:55,61 (-in required,
//     "Specifiy -in"), :68-74 (<prefix> = -out or basename of -in), src/main.cpp:30-37
//     (-version / -v), :39-48 (error -> "EXCEPTION: ..." on stdout, exit code 1),
//     README.md:45-50 (FASTA/FASTQ, gzipped or not, or a file listing input files),
//     README.md:62-72 (>id LN:i: KC:i: km:f: header), scripts/convertToGFA.py:74,36-49 (GFA).
//   ./bcalm -in <prefix>.h5 -kmer-size 31 -skip-bcalm -skip-bglue -redo-links [-gfa]
//     scripts/pufferize.py:61,143 and split_unitigs.py: their pieces carry no links; this mode reads <prefix>.unitigs.fa,
//     recomputes the L: tokens of its records (cdbg_load_unitigs + cdbg_link) and rewrites the file in place.
//   ./bcalm -in <prefix|file.unitigs.fa> -kmer-size 31 -query queries.fa[.gz] [-out prefix]
//     reads <prefix>.unitigs.fa, looks every k-mer of the query sequences up in it (cdbg_load_unitigs + cdbg_index + cdbg_query) and
//     writes <prefix>.query.tsv: name, k-mers, k-mers found, runs qpos:len:unitig:strand:upos.
//   ./bcalm -in <prefix|file.unitigs.fa> -kmer-size 31 -quantify sample.fq[.gz] [-all-abundance-counts] [-out prefix]
//     reads <prefix>.unitigs.fa, counts the k-mers of the sample at the unitig positions that spell them (cdbg_load_unitigs + cdbg_quantify +
//     cdbg_fetch_quant) and writes <prefix>.quant.tsv: unitig, k-mers, KC, covered k-mers, km [, the per-position counts].
//   ./bcalm -in <prefix|file.unitigs.fa> -kmer-size 31 -thread queries.fa[.gz] [-out prefix]
//     as -query, with the runs computed on the device (cdbg_load_unitigs + cdbg_index + cdbg_thread + cdbg_fetch_runs): writes
//     <prefix>.thread.tsv in the line format of <prefix>.query.tsv.
//   ./bcalm -in <prefix|file.unitigs.fa> -kmer-size 31 -colors samples.txt [-out prefix]
//     reads <prefix>.unitigs.fa and the sample files samples.txt names, one per non-empty line (line i is colour i; FASTA / FASTQ, plain or
//     gzip), marks every sample's k-mers at the unitig positions that spell them (cdbg_load_unitigs + cdbg_color_open + cdbg_color +
//     cdbg_color_classes) and writes <prefix>.colors.tsv (unitig, offset, len, class per run) and <prefix>.color_classes.tsv.
//     With -color-query <file> [-color-share num/den] [-color-share-of-found] it then asks which samples every sequence of <file> belongs
//     to (cdbg_color_query) and writes <prefix>.color_query.tsv: name, k-mers, k-mers found, colours reported, their indices.
//   ./bcalm -in <prefix|file.unitigs.fa> -kmer-size 31 -components [-out prefix]
//     reads <prefix>.unitigs.fa, labels the connected components of its records' graph (cdbg_load_unitigs + cdbg_components +
//     cdbg_fetch_components; links recomputed from the sequences) and writes <prefix>.components.tsv and <prefix>.unitig_components.tsv.
// Everything between parsing and writing is three calls into libcdbg.so (include/cdbg.h):
// this file is the replacement for bcalm_1::execute()/Functor (src/bcalm_1.cpp:49-97).
#include <zlib.h>

#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <algorithm>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "cdbg.h"
#include "pgz.h"

#ifndef CDBG_VERSION
#define CDBG_VERSION "cdbg-mi355x r1 (CLI-compatible with BCALM 2 v2.2.3)"
#endif

namespace {

struct Options {
    std::string in, out;
    int k = 31, amin = 2, m = 0, device = 0, log_np = -1, n_gpus = 1, cores = 0;
    bool gfa = false, verbose = false, all_ab = false, no_stream = false;
    bool redo_links = false, skip_bcalm = false, skip_bglue = false;   // -redo-links: only the link step, on an existing <prefix>.unitigs.fa
    std::string solid_out;
    std::string quantify;                            // -quantify <file>: count the k-mers of its sequences per unitig of an existing <prefix>.unitigs.fa
    std::string thread;                              // -thread <file>: the runs of its sequences' k-mers along the unitigs of an existing <prefix>.unitigs.fa
    std::string colors;                              // -colors <list>: one sample file per line; colour the unitigs of an existing <prefix>.unitigs.fa by sample
    std::string color_query;                         // -color-query <file> (with -colors): which samples every sequence of the file belongs to
    uint32_t share_num = 0, share_den = 1;           // -color-share num/den: a colour is reported when it holds at least that share of the sequence's k-mers (0/1: any)
    bool share_of_found = false;                     // -color-share-of-found: ... of the k-mers found in the graph, not of all of them
    bool components = false;                         // -components: the connected components of the records of an existing <prefix>.unitigs.fa
    std::string query;                               // -query <file>: look the k-mers of its sequences up in an existing <prefix>.unitigs.fa
};

[[noreturn]] void usage_error(const std::string& msg) { throw std::runtime_error(msg); }
void put_km(std::string& d, double km) { char t[48]; const int n = snprintf(t, sizeof t, "%.1f", km); d.append(t, (size_t)n); }   // the reference's %.1f

Options parse(int argc, char** argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) usage_error(std::string("option ") + name + " needs a value");
            return argv[++i];
        };
        if (a == "-in") o.in = need("-in");
        else if (a == "-out") o.out = need("-out");
        else if (a == "-kmer-size") o.k = atoi(need("-kmer-size"));
        else if (a == "-abundance-min") o.amin = atoi(need("-abundance-min"));
        else if (a == "-minimizer-size") o.m = atoi(need("-minimizer-size"));
        else if (a == "-device") o.device = atoi(need("-device"));
        else if (a == "-log2-partitions") o.log_np = atoi(need("-log2-partitions"));
        else if (a == "-nb-gpus") o.n_gpus = atoi(need("-nb-gpus"));   // the GPU path's counterpart of -nb-cores: GPUs of this node (power of two)
        else if (a == "-gfa") o.gfa = true;
        else if (a == "-redo-links") o.redo_links = true;             // the reference's hidden option: scripts/pufferize.py:143 tells its users to run it
        else if (a == "-query") o.query = need("-query");
        else if (a == "-quantify") o.quantify = need("-quantify");
        else if (a == "-thread") o.thread = need("-thread");
        else if (a == "-components") o.components = true;
        else if (a == "-colors") o.colors = need("-colors");
        else if (a == "-color-query") o.color_query = need("-color-query");
        else if (a == "-color-share-of-found") o.share_of_found = true;
        else if (a == "-color-share") {                               // num/den, two decimal numbers, 0 <= num <= den <= 2^32 - 1, den >= 1
            const std::string v = need("-color-share");
            const size_t sl = v.find('/');
            const std::string a0 = v.substr(0, sl), a1 = sl == std::string::npos ? "" : v.substr(sl + 1);
            auto digits = [](const std::string& t) { return !t.empty() && t.size() <= 10 && t.find_first_not_of("0123456789") == std::string::npos; };
            const unsigned long long nu = digits(a0) ? strtoull(a0.c_str(), nullptr, 10) : ~0ull, de = digits(a1) ? strtoull(a1.c_str(), nullptr, 10) : ~0ull;
            if (nu > 0xFFFFFFFFull || de > 0xFFFFFFFFull || de < 1 || nu > de) usage_error("malformed -color-share '" + v + "': num/den with 0 <= num <= den, den >= 1");
            o.share_num = (uint32_t)nu; o.share_den = (uint32_t)de;
        }
        else if (a == "-skip-bcalm") o.skip_bcalm = true;
        else if (a == "-skip-bglue") o.skip_bglue = true;
        else if (a == "-no-stream-scan") o.no_stream = true;           // dev: do not announce the input volume (the read scan starts when the text is complete)
        else if (a == "-all-abundance-counts") o.all_ab = true;        // README.md:74-80
        else if (a == "-solid-kmers-out") o.solid_out = need("-solid-kmers-out");   // hidden in the reference (bcalm_1.cpp:37)
        else if (a == "-verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') ++i; }
        else if (a == "-nb-cores") o.cores = atoi(need("-nb-cores"));   // README.md / gatb option: here the host threads that parse the input and format the output (0 = all, at most 32)
        else if (a == "-max-memory" || a == "-max-disk" || a == "-out-tmp" || a == "-out-dir" ||
                 a == "-repartition-type" || a == "-minimizer-type" || a == "-histo-max" || a == "-solidity-kind")
            need(a.c_str());                     // accepted for CLI compatibility; meaningless on the GPU path
        else usage_error("Unknown parameter '" + a + "'");
    }
    return o;
}

std::string base_name(const std::string& path) {          // strip directory and the last extension
    size_t s = path.find_last_of('/');
    std::string b = s == std::string::npos ? path : path.substr(s + 1);
    size_t d = b.find_last_of('.');
    if (d != std::string::npos && d > 0) b = b.substr(0, d);
    if (b.size() > 3 && b.substr(b.size() - 3) == ".fa") b = b.substr(0, b.size() - 3);   // reads.fa.gz -> reads
    return b;
}

// ---- ingest (README.md:45-50: FASTA / FASTQ, gzipped or not, or a file listing input files) ----
// N parser threads write sequence text STRAIGHT INTO the library's pinned staging buffers (cdbg_stage_acquire / _commit: no
// intermediate copy; the H2D copies and -- with cdbg_expect_input -- the read scan itself run behind the parsing).  A plain
// file is memory-mapped and cut into record-aligned slices (FASTA: at "\n>", strict four-line FASTQ: at an '@' line whose
// second successor starts with '+'), one task per slice; a FASTQ whose records wrap is one task.  A gzip file is inflated by ALL
// threads when there are few of them (pgz.h: block starts searched, chunks decoded with the window unknown, resolved in order) and
// its text parsed in slices like a plain file; a list of many gzip files keeps one zlib stream per thread in flight instead.
struct Ingest {
    std::vector<cdbg_ctx*> ctxs; int k = 31;
    std::atomic<size_t> next_ctx{0};
    std::atomic<uint64_t> n_seq{0}, n_bases{0};
    std::mutex err_mu; std::string error; std::atomic<bool> failed{false}, irregular{false};
    void fail(const std::string& e) { std::lock_guard<std::mutex> l(err_mu); if (error.empty()) error = e; failed = true; }
};
// one per parser thread: the staging buffer being filled.  A sequence that does not fit is continued in the next buffer
// with its last k-1 bases repeated (every k-mer across the cut is seen exactly once).
class Sink {
    Ingest& I; cdbg_ctx* ctx = nullptr; char* buf = nullptr; uint64_t cap = 0, fill = 0, cur = 0;   // cur: bases of the open sequence in this buffer
    void acquire() {
        ctx = I.ctxs[I.next_ctx.fetch_add(1) % I.ctxs.size()];      // (several GPUs: whole buffers of complete sequences go to the contexts in turn)
        if (cdbg_stage_acquire(ctx, &buf, &cap) != 0) { buf = nullptr; throw std::runtime_error(cdbg_last_error()); }
        fill = 0; cur = 0;
    }
    void commit() {
        if (!buf) return;
        char* b = buf; buf = nullptr;
        if (cdbg_stage_commit(ctx, b, fill) != 0) throw std::runtime_error(cdbg_last_error());
    }
public:
    uint64_t n_seq = 0, n_bases = 0;
    explicit Sink(Ingest& i) : I(i) {}
    void bases(const char* p, size_t n) {
        n_bases += n;
        while (n) {
            if (!buf) acquire();
            const uint64_t room = cap - 1 - fill;                  // (the last byte is kept for the separator)
            if (!room) {
                const uint64_t t = std::min<uint64_t>(cur, (uint64_t)I.k - 1);
                std::string tail(buf + fill - t, t);
                if (cur < (uint64_t)I.k) fill -= cur;              // (fewer than k bases of it here: the whole piece moves on)
                buf[fill++] = '\n';
                commit(); acquire();
                memcpy(buf, tail.data(), t); fill = t; cur = t;
                continue;
            }
            const size_t take = (size_t)std::min<uint64_t>(room, n);
            memcpy(buf + fill, p, take); fill += take; cur += take; p += take; n -= take;
        }
    }
    void end_seq() {                                               // (cap - 1 >= fill always: there is room)
        if (buf && fill && buf[fill - 1] != '\n') buf[fill++] = '\n';
        cur = 0;
        if (buf && cap - fill < (1u << 16)) commit();               // nearly full: send it while the boundary is clean
    }
    void finish() { end_seq(); if (buf) commit(); I.n_seq += n_seq; I.n_bases += n_bases; n_seq = n_bases = 0; }
    ~Sink() { if (buf) cdbg_stage_commit(ctx, buf, 0); }           // (error path: hand the buffer back unused)
};
inline size_t line_len(const char* p, const char* end) { const char* e = (const char*)memchr(p, '\n', (size_t)(end - p)); return e ? (size_t)(e - p) : (size_t)(end - p); }
inline size_t rstrip_cr(const char* p, size_t n) { while (n && p[n - 1] == '\r') --n; return n; }

// a record-aligned slice of a memory-mapped plain file: FASTA (wrapped or not) ...
void parse_fasta_slice(const char* p, const char* end, Sink& out) {
    while (p < end) {
        const size_t n = line_len(p, end), m = rstrip_cr(p, n);
        if (m && p[0] == '>') { out.end_seq(); ++out.n_seq; }
        else if (m && p[0] != ';') out.bases(p, m);
        p += n + 1;
    }
    out.end_seq();
}
// ... or strict four-line FASTQ; returns false when a record is not of that shape (the caller falls back to the tolerant serial parser)
bool parse_fastq4_slice(const char* p, const char* end, Sink& out) {
    while (p < end) {
        const size_t n0 = line_len(p, end);
        if (!rstrip_cr(p, n0)) { p += n0 + 1; continue; }          // blank line between records
        const char* s = p + n0 + 1; if (s >= end || p[0] != '@') return false;
        const size_t n1 = line_len(s, end);
        const char* pl = s + n1 + 1; if (pl >= end || pl[0] != '+') return false;
        const size_t n2 = line_len(pl, end);
        const char* q = pl + n2 + 1; if (q > end) return false;
        const size_t n3 = q < end ? line_len(q, end) : 0;
        const size_t m1 = rstrip_cr(s, n1);
        if (rstrip_cr(q, n3) != m1) return false;
        out.bases(s, m1); out.end_seq(); ++out.n_seq;
        p = q + n3 + 1;
    }
    return true;
}
// the tolerant serial parser: FASTA / FASTQ, plain or gzip (zlib reads both), FASTQ records may wrap their sequence and quality
// over several lines (README.md:45-50 accepts any FASTQ): after the '@' header the sequence runs until the '+' line, the
// quality until it is as long as the sequence
void parse_stream(const std::string& path, Sink& out) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) usage_error("cannot open input file " + path);
    gzbuffer(f, 1 << 20);
    std::vector<char> line(1 << 22);
    int fmt = 0;                                // 0 unknown, 1 FASTA, 2 FASTQ
    int fq_state = 0; char fq_kind = 0; uint64_t fq_seq = 0, fq_qual = 0;   // state: 0 header expected, 1 sequence, 2 quality
    bool partial = false;                       // previous gzgets returned an unterminated piece
    while (gzgets(f, line.data(), (int)line.size())) {
        size_t n = strlen(line.data());
        const bool complete = n && line[n - 1] == '\n';
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) --n;
        const bool starts_line = !partial;
        partial = !complete;
        if (fmt == 0 && starts_line && n) fmt = line[0] == '@' ? 2 : 1;
        if (fmt == 2) {
            if (starts_line) {
                if (fq_state == 0) {
                    if (!n) fq_kind = 0;
                    else if (line[0] == '@') fq_kind = 'H';
                    else { gzclose(f); usage_error("malformed FASTQ record in " + path + " (sequence " + std::to_string(out.n_seq + 1) + "): '@' expected"); }
                } else if (fq_state == 1) fq_kind = (n && line[0] == '+') ? 'P' : 'S';
                else fq_kind = 'Q';
            }
            if (fq_kind == 'S') { out.bases(line.data(), n); fq_seq += n; }
            else if (fq_kind == 'Q') fq_qual += n;
            if (complete) {
                if (fq_kind == 'H') { fq_state = 1; fq_seq = 0; }
                else if (fq_kind == 'P') { out.end_seq(); ++out.n_seq; fq_state = 2; fq_qual = 0; }
                else if (fq_kind == 'Q' && fq_qual >= fq_seq) fq_state = 0;
            }
        } else {
            if (starts_line && n && line[0] == '>') { out.end_seq(); ++out.n_seq; }
            else if (!(starts_line && n && line[0] == ';')) out.bases(line.data(), n);
        }
    }
    int zerr = Z_OK; const char* zmsg = gzerror(f, &zerr);
    if (zerr != Z_OK && zerr != Z_STREAM_END) { const std::string m = zmsg ? zmsg : "read error"; gzclose(f); usage_error(path + ": " + m); }
    gzclose(f);
    out.end_seq();
}

struct Mapped {                                  // a plain file, memory-mapped read-only
    const char* p = nullptr; size_t n = 0; int fd = -1;
    bool open(const std::string& path) {
        fd = ::open(path.c_str(), O_RDONLY); if (fd < 0) return false;
        struct stat st; if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) { ::close(fd); fd = -1; return false; }
        n = (size_t)st.st_size;
        void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { ::close(fd); fd = -1; return false; }
        p = (const char*)m; (void)madvise(m, n, MADV_WILLNEED);
        return true;
    }
    ~Mapped() { if (p) munmap((void*)p, n); if (fd >= 0) ::close(fd); }
};
struct Task { int kind; std::string path; std::shared_ptr<Mapped> map; size_t beg = 0, end = 0; };   // kind: 0 serial stream, 1 FASTA slice, 2 four-line FASTQ slice
bool is_gzip(const std::string& path) {
    FILE* raw = fopen(path.c_str(), "rb"); unsigned char magic[2] = {0, 0};
    if (raw) { if (fread(magic, 1, 2, raw) != 2) magic[0] = 0; fclose(raw); }
    return magic[0] == 0x1f && magic[1] == 0x8b;
}
// start of the first record at or after `pos`
size_t next_fasta_record(const char* p, size_t n, size_t pos) {
    if (pos == 0) return 0;
    for (size_t i = pos - 1; i + 1 < n;) {
        const char* e = (const char*)memchr(p + i, '\n', n - i);
        if (!e) return n;
        i = (size_t)(e - p) + 1;
        if (i < n && p[i] == '>') return i;
    }
    return n;
}
size_t next_fastq4_record(const char* p, size_t n, size_t pos) {
    if (pos == 0) return 0;
    const char* e = (const char*)memchr(p + pos - 1, '\n', n - (pos - 1));
    if (!e) return n;
    size_t i = (size_t)(e - p) + 1;
    for (int tries = 0; tries < 8 && i < n; ++tries) {            // a line that starts with '@' and whose second successor starts with '+' is a header: a
        const size_t l0 = line_len(p + i, p + n);                  // quality line that starts with '@' is followed by a header and a SEQUENCE line
        const size_t j = i + l0 + 1; if (j >= n) return n;
        const size_t l1 = line_len(p + j, p + n);
        const size_t h = j + l1 + 1;
        if (p[i] == '@' && h < n && p[h] == '+') return i;
        i = j;
    }
    return n;                                                      // (no record start found: the previous slice's parser will say "irregular")
}
void plan_file(const std::string& path, int threads, std::vector<Task>& tasks) {
    if (!is_gzip(path)) {
        auto mp = std::make_shared<Mapped>();
        if (mp->open(path)) {
            const char* p = mp->p; const size_t n = mp->n;
            size_t f0 = 0; while (f0 < n && (p[f0] == '\n' || p[f0] == '\r')) ++f0;
            int kind = 0;
            if (f0 < n && (p[f0] == '>' || p[f0] == ';')) kind = 1;
            else if (f0 < n && p[f0] == '@') {                     // strict four-line FASTQ? (judged by its first record; a slice that finds otherwise reports it)
                const size_t l0 = line_len(p + f0, p + n), s1 = f0 + l0 + 1;
                if (s1 < n) { const size_t l1 = line_len(p + s1, p + n), s2 = s1 + l1 + 1;
                    if (s2 < n && p[s2] == '+') { const size_t l2 = line_len(p + s2, p + n), s3 = s2 + l2 + 1;
                        if (s3 <= n && rstrip_cr(p + s3, s3 < n ? line_len(p + s3, p + n) : 0) == rstrip_cr(p + s1, l1)) kind = 2; } }
            }
            if (kind) {
                size_t slice = std::max<size_t>(n / (size_t)(threads * 4) + 1, 8u << 20);   // a few slices per thread, none below 8 MB
                if (const char* e = getenv("BCALM_SLICE_BYTES")) slice = std::max<size_t>(1, strtoull(e, nullptr, 10));   // (tests: many slices of a small file)
                size_t beg = 0;
                while (beg < n) {
                    size_t end = beg + slice >= n ? n : (kind == 1 ? next_fasta_record(p, n, beg + slice) : next_fastq4_record(p, n, beg + slice));
                    if (end <= beg) end = n;
                    tasks.push_back(Task{ kind, path, mp, beg, end });
                    beg = end;
                }
                return;
            }
        }
    }
    tasks.push_back(Task{ 0, path, nullptr, 0, 0 });
}
// CPUs this process may really use: the affinity mask and the container's CPU quota (cgroup v2 cpu.max, v1 cfs_quota_us / cfs_period_us), not the
// machine's thread count -- a 256-thread host that grants 16 CPUs runs 32 parser threads slower than 16 (profiles/r06_gz_ingest_parallel_inflate.log)
unsigned usable_cpus() {
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set; CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) n = std::min<unsigned>(n, (unsigned)c); }
    long long quota = -1, period = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64] = {0}; if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else {
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &quota) != 1) quota = -1; fclose(g); }
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &period) != 1) period = 0; fclose(g); }
    }
    if (quota > 0 && period > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
    return n;
}
bool ingest_gz_parallel(Ingest& I, const std::string& path, int threads);
// parse every file with `threads` workers; false: a FASTQ file was not as regular as its first record promised (nothing usable was pushed)
bool ingest_files(Ingest& I, const std::vector<std::string>& files, int threads, bool allow_slices) {
    std::vector<Task> tasks;
    // few gzip files and many threads: each is inflated by all threads, one after the other (pgz.h); many gzip files: one thread each, as before
    std::vector<std::string> gz_parallel;
    size_t n_gz = 0; for (const auto& f : files) n_gz += is_gzip(f);
    const bool pgz_on = allow_slices && threads >= 2 && n_gz * 2 <= (size_t)threads && getenv("BCALM_GZ_SERIAL") == nullptr;
    for (const auto& f : files) {
        if (pgz_on && is_gzip(f)) gz_parallel.push_back(f);
        else if (allow_slices) plan_file(f, threads, tasks);
        else tasks.push_back(Task{ 0, f, nullptr, 0, 0 });
    }
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        try {
            Sink out(I);
            for (;;) {
                const size_t t = next.fetch_add(1);
                if (t >= tasks.size() || I.failed || I.irregular) break;
                const Task& T = tasks[t];
                if (T.kind == 0) parse_stream(T.path, out);
                else if (T.kind == 1) parse_fasta_slice(T.map->p + T.beg, T.map->p + T.end, out);
                else if (!parse_fastq4_slice(T.map->p + T.beg, T.map->p + T.end, out)) { I.irregular = true; break; }
            }
            out.finish();
        } catch (const std::exception& e) { I.fail(e.what()); }
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, tasks.size()));
    std::vector<std::thread> th;
    for (int i = 1; i < nt; ++i) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    if (I.failed) usage_error(I.error);
    for (const auto& f : gz_parallel) {
        if (I.irregular) break;
        if (!ingest_gz_parallel(I, f, threads)) { Sink out(I); parse_stream(f, out); out.finish(); }
    }
    return !I.irregular;
}

// ---- one gzip file inflated by all threads (pgz.h): real read sets ship as one or two .fastq.gz, and zlib inflates a file with one thread ----
// start of the last record of [p, p + n) that may be incomplete (n: every record is complete); 0: no record start known
size_t last_fasta_start(const char* p, size_t n) {
    for (size_t e = n; e > 1;) {
        const char* q = (const char*)memrchr(p, '>', e); if (!q) return 0;
        const size_t i = (size_t)(q - p);
        if (i == 0 || p[i - 1] == '\n') return i;
        e = i;
    }
    return 0;
}
size_t last_fastq4_start(const char* p, size_t n) {
    for (size_t back = (size_t)1 << 20;; back *= 16) {
        const size_t from = n > back ? n - back : 0;
        size_t r = from ? next_fastq4_record(p, n, from) : 0;
        if (r < n) {
            for (;;) {                                              // whole records from r on: four lines each
                while (r < n && (p[r] == '\n' || p[r] == '\r')) ++r;
                size_t e = r; int lines = 0;
                while (lines < 4) { const char* nl = (const char*)memchr(p + e, '\n', n - e); if (!nl) break; e = (size_t)(nl - p) + 1; ++lines; }
                if (lines < 4) return r;
                r = e;
            }
        }
        if (!from) return 0;
    }
}
struct IrregularInput {};
// false: not handled, nothing was pushed (the caller parses the file with zlib)
bool ingest_gz_parallel(Ingest& I, const std::string& path, int threads) {
    Mapped mp; if (!mp.open(path)) return false;
    // 4 MB of compressed bytes per chunk (its text is held as 16-bit symbols until the wave is resolved); smaller for a small file, so that every thread gets some
    size_t chunk = std::min<size_t>((size_t)4 << 20, std::max<size_t>((size_t)1 << 20, mp.n / ((size_t)threads * 4) + 1));
    if (const char* e = getenv("BCALM_GZ_CHUNK")) chunk = std::max<size_t>(1024, strtoull(e, nullptr, 10));   // (tests: many chunks of a small file)
    std::vector<std::unique_ptr<Sink>> sinks;
    for (int t = 0; t < threads; ++t) sinks.emplace_back(new Sink(I));
    int fmt = 0;                                                    // 1 FASTA, 2 strict four-line FASTQ
    auto on_wave = [&](char* p, size_t n, bool last) -> size_t {
        if (!fmt) {
            size_t f0 = 0; while (f0 < n && (p[f0] == '\n' || p[f0] == '\r')) ++f0;
            if (f0 < n && (p[f0] == '>' || p[f0] == ';')) fmt = 1;
            else if (f0 < n && p[f0] == '@') {                     // (plan_file's test of the first record)
                const size_t l0 = line_len(p + f0, p + n), s1 = f0 + l0 + 1;
                if (s1 < n) { const size_t l1 = line_len(p + s1, p + n), s2 = s1 + l1 + 1;
                    if (s2 < n && p[s2] == '+') { const size_t l2 = line_len(p + s2, p + n), s3 = s2 + l2 + 1;
                        if (s3 <= n && rstrip_cr(p + s3, s3 < n ? line_len(p + s3, p + n) : 0) == rstrip_cr(p + s1, l1)) fmt = 2; } }
            }
            if (!fmt) return pgz::ABORT;
        }
        const size_t cut = last ? n : (fmt == 1 ? last_fasta_start(p, n) : last_fastq4_start(p, n));
        if (!cut) return n;                                         // not one complete record yet: all of it again, with more behind
        std::vector<size_t> b((size_t)threads + 1, cut); b[0] = 0;
        for (int t = 1; t < threads; ++t) {
            const size_t pos = cut / (size_t)threads * (size_t)t;
            const size_t x = pos ? (fmt == 1 ? next_fasta_record(p, cut, pos) : next_fastq4_record(p, cut, pos)) : 0;
            b[t] = std::min(cut, std::max(x, b[t - 1]));
        }
        std::atomic<bool> irregular{false};
        pgz::parallel_for((size_t)threads, threads, [&](size_t t) {
            if (b[t] >= b[t + 1] || I.failed) return;
            try {
                if (fmt == 1) parse_fasta_slice(p + b[t], p + b[t + 1], *sinks[t]);
                else if (!parse_fastq4_slice(p + b[t], p + b[t + 1], *sinks[t])) irregular = true;
            } catch (const std::exception& e) { I.fail(e.what()); }
        });
        if (I.failed) throw std::runtime_error(I.error);
        if (irregular) throw IrregularInput{};
        return n - cut;
    };
    pgz::Stats st; int rc = 0;
    try { rc = pgz::inflate_parallel((const uint8_t*)mp.p, mp.n, threads, chunk, on_wave, &st); }
    catch (const IrregularInput&) { I.irregular = true; return true; }         // (records that are not four lines: the caller starts over)
    catch (const std::exception& e) { usage_error(path + ": " + e.what()); }
    if (rc != 0) return false;
    for (auto& sk : sinks) sk->finish();
    if (getenv("BCALM_GZ_VERBOSE")) fprintf(stderr, "[bcalm] %s: inflated by %d threads, %zu chunks (%zu block starts found), %zu waves, %zu members, %.2f GB of text; find %.2f s, decode %.2f s, resolve %.2f s; parse %.2f s beside the decoding, %.2f s of it waited for\n",
                                            path.c_str(), threads, st.chunks, st.starts_found, st.waves, st.members, st.out_bytes * 1e-9, st.s_find, st.s_decode, st.s_resolve, st.s_caller, st.s_wait);
    return true;
}

// approximate number of sequence bytes a file will deliver (cdbg_expect_input): gzip ~4x, FASTQ carries as many quality bytes
uint64_t estimate_text_bytes(const std::string& path) {
    struct stat st; if (stat(path.c_str(), &st) != 0) return 0;
    uint64_t n = (uint64_t)st.st_size;
    gzFile f = gzopen(path.c_str(), "rb"); char c0 = 0;
    if (f) { const int c = gzgetc(f); if (c >= 0) c0 = (char)c; gzclose(f); }
    FILE* raw = fopen(path.c_str(), "rb"); unsigned char magic[2] = {0, 0};
    if (raw) { if (fread(magic, 1, 2, raw) != 2) magic[0] = 0; fclose(raw); }
    if (magic[0] == 0x1f && magic[1] == 0x8b) n *= 4;
    if (c0 == '@') n /= 2;
    return n + n / 50 + (1 << 20);
}

bool looks_like_file_list(const std::string& path) {       // README.md:47-50 "ls -1 *.fastq > list_reads"
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[4096]; bool is_list = false;
    if (gzgets(f, buf, sizeof buf)) {
        size_t n = strlen(buf); while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) buf[--n] = 0;
        if (n && buf[0] != '>' && buf[0] != '@' && buf[0] != ';') { gzFile g = gzopen(buf, "rb"); if (g) { is_list = true; gzclose(g); } }
    }
    gzclose(f);
    return is_list;
}

void check(int rc) { if (rc != 0) throw std::runtime_error(cdbg_last_error()); }

// ---- -redo-links: the link step alone, on the records of an existing <prefix>.unitigs.fa (any FASTA: sequences may wrap) ----
struct FaRecord { std::string rest; size_t seq_off = 0, seq_len = 0; };   // rest: the header after its first word; the sequence lies in the slice's `bases`
struct FaSlice { std::vector<FaRecord> recs; std::string bases; };
void parse_unitig_slice(const char* p, const char* end, FaSlice& out) {
    bool have = false;
    while (p < end) {
        const size_t n = line_len(p, end), m = rstrip_cr(p, n);
        if (m && p[0] == '>') {
            FaRecord r; r.seq_off = out.bases.size();
            const char* sp = (const char*)memchr(p, ' ', m);
            if (sp) r.rest.assign(sp + 1, (size_t)(p + m - sp - 1));
            out.recs.push_back(std::move(r)); have = true;
        } else if (m && p[0] != ';' && have) {
            size_t a = 0, b = m;                                   // (blanks around a sequence line are not bases)
            while (a < b && (p[a] == ' ' || p[a] == '\t')) ++a;
            while (b > a && (p[b - 1] == ' ' || p[b - 1] == '\t')) --b;
            out.bases.append(p + a, b - a); out.recs.back().seq_len += b - a;
        } else if (m && p[0] != ';') usage_error("sequence data before the first '>' header");
        p += n + 1;
    }
}
// header tokens to keep: everything after the first word but the L: tokens, in order (tokens are separated by single blanks, as scripts/convertToGFA.py:77 splits them)
void kept_tokens(const std::string& rest, std::vector<std::string>& out) {
    out.clear();
    size_t p = 0;
    while (p <= rest.size()) {
        size_t q = rest.find(' ', p); if (q == std::string::npos) q = rest.size();
        if (q > p && rest.compare(p, 2, "L:") != 0) out.emplace_back(rest, p, q - p);
        p = q + 1;
    }
}
// the records of a unitigs file in file order -- one arena of bases, offsets, the headers -- as cdbg_load_unitigs takes them (-redo-links and -query)
struct UnitigFile {
    std::shared_ptr<Mapped> mp; std::vector<FaSlice> slices;
    uint64_t nu = 0, tb = 0; std::unique_ptr<char[]> seq; std::vector<uint64_t> off; std::vector<const std::string*> rest;
};
void read_unitig_file(const Options& o, const std::string& fa, int threads, const char* mode, UnitigFile& F) {
    F.mp = std::make_shared<Mapped>();
    auto& mp = F.mp; auto& slices = F.slices;
    { struct stat sb; if (stat(fa.c_str(), &sb) != 0) usage_error(std::string(mode) + ": cannot open " + fa + " (the unitigs of an earlier run are expected there)"); }
    if (mp->open(fa)) {                                            // (false: an empty file -- no records)
        const char* p = mp->p; const size_t n = mp->n;
        size_t slice = std::max<size_t>(n / (size_t)(threads * 4) + 1, 8u << 20);
        if (const char* e = getenv("BCALM_SLICE_BYTES")) slice = std::max<size_t>(1, strtoull(e, nullptr, 10));
        std::vector<std::pair<size_t, size_t>> cuts;
        for (size_t beg = 0; beg < n;) {
            size_t end = beg + slice >= n ? n : next_fasta_record(p, n, beg + slice);
            if (end <= beg) end = n;
            cuts.emplace_back(beg, end); beg = end;
        }
        slices.resize(cuts.size());
        std::mutex em; std::string err;
        pgz::parallel_for(cuts.size(), threads, [&](size_t i) {
            try { parse_unitig_slice(p + cuts[i].first, p + cuts[i].second, slices[i]); }
            catch (const std::exception& e) { std::lock_guard<std::mutex> l(em); if (err.empty()) err = e.what(); }
        });
        if (!err.empty()) usage_error(fa + ": " + err);
    }
    // records in file order: one arena, offsets, the headers
    uint64_t nu = 0, tb = 0;
    for (const FaSlice& sl : slices) { nu += sl.recs.size(); tb += sl.bases.size(); }
    F.nu = nu; F.tb = tb;
    F.seq.reset(new char[tb + 1]);
    F.off.assign(nu + 1, 0); F.rest.assign(nu ? nu : 1, nullptr);
    {
        uint64_t i = 0, w = 0;
        for (const FaSlice& sl : slices) {
            if (!sl.bases.empty()) memcpy(F.seq.get() + w, sl.bases.data(), sl.bases.size());
            for (const FaRecord& r : sl.recs) {
                if (r.seq_len < (size_t)o.k) usage_error(fa + ": record " + std::to_string(i) + " has " + std::to_string(r.seq_len) + " bases, fewer than k = " + std::to_string(o.k));
                F.off[i] = w + r.seq_off; F.rest[i] = &r.rest; ++i;
            }
            w += sl.bases.size();
        }
        F.off[nu] = tb;
    }
}
cdbg_ctx* load_unitig_file(const Options& o, const std::string& fa, UnitigFile& F, const uint64_t* kc = nullptr) {
    cdbg_params prm{}; prm.k = o.k; prm.abundance_min = std::max(1, o.amin); prm.minimizer_size = 0; prm.log2_partitions = -1; prm.device_id = o.device; prm.world_size = 1;
    cdbg_ctx* ctx = nullptr; check(cdbg_create(&prm, &ctx));
    if (cdbg_load_unitigs(ctx, F.seq.get(), F.off.data(), F.nu, kc) != 0) {
        const std::string e = cdbg_last_error(); unsigned long long u = 0;
        cdbg_destroy(ctx);
        if (sscanf(e.c_str(), "unitig %llu", &u) == 1) usage_error(fa + ": record " + std::to_string(u) + ": " + e);
        usage_error(fa + ": " + e);
    }
    return ctx;
}
int redo_links(const Options& o, const std::string& prefix, int threads) {
    auto t0 = std::chrono::steady_clock::now();
    const std::string fa = prefix + ".unitigs.fa";
    UnitigFile F; read_unitig_file(o, fa, threads, "-redo-links", F);
    auto& mp = F.mp; const uint64_t nu = F.nu, tb = F.tb; auto& seq = F.seq; auto& off = F.off; auto& rest = F.rest;
    cdbg_ctx* ctx = load_unitig_file(o, fa, F);
    struct Guard { cdbg_ctx* c; ~Guard() { cdbg_destroy(c); } } guard{ ctx };
    check(cdbg_link(ctx));
    uint64_t nl = 0; check(cdbg_num_links(ctx, &nl));
    std::vector<uint64_t> loff(2 * nu + 1), kc(nu ? nu : 1); std::vector<uint32_t> lto(nl ? nl : 1);
    check(cdbg_fetch_links(ctx, loff.data(), lto.data()));
    { uint64_t n2 = 0, t2 = 0; check(cdbg_num_unitigs(ctx, &n2, &t2)); if (n2 != nu || t2 != tb) usage_error("internal: the loaded set differs from the file");
      check(cdbg_fetch_unitigs(ctx, 0, nu, seq.get(), off.data(), kc.data())); }                       // (the library's copy: upper case)
    // written beside the original and renamed over it: a failure leaves the file as it was
    const std::string gfa_name = prefix + ".unitigs.gfa";
    struct TmpOut {                                                // a temporary file: closed and removed on every way out but commit()
        std::string name; FILE* f = nullptr;
        ~TmpOut() { if (f) fclose(f); if (!name.empty()) remove(name.c_str()); }
        void open(const std::string& n) { f = fopen(n.c_str(), "w"); if (!f) usage_error("cannot write " + n); name = n; }
        bool close() { FILE* g = f; f = nullptr; return !g || fclose(g) == 0; }
        bool commit(const std::string& to) { if (rename(name.c_str(), to.c_str()) != 0) return false; name.clear(); return true; }
    } tfa, tgfa;
    tfa.open(fa + ".tmp" + std::to_string((long)getpid()));
    if (o.gfa) tgfa.open(gfa_name + ".tmp" + std::to_string((long)getpid()));
    FILE* const out = tfa.f; FILE* const gfa = tgfa.f;
    if (gfa) fprintf(gfa, "H\tVN:Z:1.0\tks:i:%d\n", o.k);
    bool wfail = false; std::string werr;
    {
        const uint64_t BLOCK = 1u << 15, nblocks = (nu + BLOCK - 1) / BLOCK;
        std::atomic<uint64_t> next_block{0};
        std::mutex wm; std::condition_variable wcv; uint64_t turn = 0;
        std::atomic<bool> stop{false};
        auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
        auto write_blocks = [&]() {
            std::string fb, gb; std::vector<std::string> toks;
            for (;;) {
                const uint64_t b = next_block.fetch_add(1);
                if (b >= nblocks || stop.load()) break;
                fb.clear(); gb.clear();
                const uint64_t i0 = b * BLOCK, i1 = std::min(nu, i0 + BLOCK);
                for (uint64_t i = i0; i < i1; ++i) {
                    const uint64_t len = off[i + 1] - off[i];
                    kept_tokens(*rest[i], toks);
                    fb.push_back('>'); put_u(fb, i);                // consecutive renumbering, as the split scripts number their pieces
                    for (const std::string& t : toks) { fb.push_back(' '); fb.append(t); }
                    if (gfa) {                                      // the S line of scripts/convertToGFA.py:35-47 for this header
                        gb.append("S\t"); put_u(gb, i); gb.push_back('\t'); gb.append(seq.get() + off[i], (size_t)len);
                        for (const std::string& t : toks) { gb.push_back('\t'); if (t.compare(0, 2, "MA") == 0) { gb.append("MA:f:"); gb.append(t, 2, std::string::npos); } else gb.append(t); }
                        while (!gb.empty() && strchr(" \t\r\f\v", gb.back())) gb.pop_back();
                        gb.push_back('\n');
                    }
                    for (int side = 1; side >= 0; --side)          // '+' links (through the last k-mer) first, then '-'; targets ascending
                        for (uint64_t j = loff[2 * i + side]; j < loff[2 * i + side + 1]; ++j) {
                            const char fs = side ? '+' : '-', ts = (lto[j] & 1u) ? '-' : '+';
                            fb.append(" L:"); fb.push_back(fs); fb.push_back(':'); put_u(fb, lto[j] >> 1); fb.push_back(':'); fb.push_back(ts);
                            if (gfa) { gb.append("L\t"); put_u(gb, i); gb.push_back('\t'); gb.push_back(fs); gb.push_back('\t'); put_u(gb, lto[j] >> 1);
                                       gb.push_back('\t'); gb.push_back(ts); gb.push_back('\t'); put_u(gb, (unsigned long long)(o.k - 1)); gb.append("M\n"); }
                        }
                    fb.append(" \n");
                    fb.append(seq.get() + off[i], (size_t)len); fb.push_back('\n');
                }
                std::unique_lock<std::mutex> l(wm);
                wcv.wait(l, [&] { return turn == b || stop.load(); });
                if (stop.load()) break;
                if (fwrite(fb.data(), 1, fb.size(), out) != fb.size()) wfail = true;
                if (gfa && fwrite(gb.data(), 1, gb.size(), gfa) != gb.size()) wfail = true;
                ++turn; wcv.notify_all();
            }
        };
        auto writer = [&]() {                                      // (an exception must not leave its thread: the others wait for this one's turn)
            try { write_blocks(); }
            catch (const std::exception& e) { std::lock_guard<std::mutex> l(wm); if (werr.empty()) werr = e.what(); stop.store(true); wcv.notify_all(); }
        };
        const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, nblocks));
        std::vector<std::thread> th;
        for (int i = 1; i < nt; ++i) th.emplace_back(writer);
        writer();
        for (auto& t : th) t.join();
    }
    if (!werr.empty()) usage_error("writing " + fa + ": " + werr);
    if (!tfa.close()) wfail = true;
    if (!tgfa.close()) wfail = true;
    if (wfail) usage_error("write error on " + tfa.name + (o.gfa ? " or " + tgfa.name : ""));
    mp.reset();                                                    // (unmap before the file is replaced)
    // the GFA first: whatever fails up to here, or in this rename, leaves <prefix>.unitigs.fa as it was
    if (o.gfa && !tgfa.commit(gfa_name)) usage_error("cannot rename " + tgfa.name + " to " + gfa_name);
    if (!tfa.commit(fa)) usage_error("cannot rename " + tfa.name + " to " + fa + (o.gfa ? " (" + gfa_name + " is already the new one)" : ""));
    printf("links recomputed: %llu unitigs, %llu links (%.2f s)\n", (unsigned long long)nu, (unsigned long long)nl,
           std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf("unitigs written to %s\n", fa.c_str());
    return EXIT_SUCCESS;
}

// ---- -query: which unitig, offset and strand holds every k-mer of the query sequences (cdbg_load_unitigs + cdbg_index + cdbg_query) ----
// the tolerant serial reader of parse_stream with the record names kept: FASTA / FASTQ, plain or gzip, sequences and qualities may wrap;
// on_seq(name) is called when a record's sequence is complete and lies at the end of `bases`
template <class F>
void parse_queries(const std::string& path, std::string& bases, F&& on_seq, const char* what = "query file") {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) usage_error(std::string("cannot open ") + what + " " + path);
    gzbuffer(f, 1 << 20);
    std::vector<char> line(1 << 22);
    int fmt = 0, fq_state = 0; char fq_kind = 0; uint64_t fq_seq = 0, fq_qual = 0;
    bool partial = false, open = false; std::string name; uint64_t n_rec = 0;
    auto first_word = [&](size_t n) { size_t e = 1; while (e < n && line[e] != ' ' && line[e] != '\t') ++e; name.assign(line.data() + 1, e - 1); };
    auto close = [&]() { if (open) { on_seq(name); open = false; } };
    while (gzgets(f, line.data(), (int)line.size())) {
        size_t n = strlen(line.data());
        const bool complete = n && line[n - 1] == '\n';
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) --n;
        const bool starts_line = !partial;
        partial = !complete;
        if (fmt == 0 && starts_line && n) fmt = line[0] == '@' ? 2 : 1;
        if (fmt == 2) {
            if (starts_line) {
                if (fq_state == 0) {
                    if (!n) fq_kind = 0;
                    else if (line[0] == '@') { fq_kind = 'H'; first_word(n); open = true; ++n_rec; }
                    else { gzclose(f); usage_error("malformed FASTQ record in " + path + " (sequence " + std::to_string(n_rec + 1) + "): '@' expected"); }
                } else if (fq_state == 1) fq_kind = (n && line[0] == '+') ? 'P' : 'S';
                else fq_kind = 'Q';
            }
            if (fq_kind == 'S') { bases.append(line.data(), n); fq_seq += n; }
            else if (fq_kind == 'Q') fq_qual += n;
            if (complete) {
                if (fq_kind == 'H') { fq_state = 1; fq_seq = 0; }
                else if (fq_kind == 'P') { close(); fq_state = 2; fq_qual = 0; }
                else if (fq_kind == 'Q' && fq_qual >= fq_seq) fq_state = 0;
            }
        } else {
            if (starts_line && n && line[0] == '>') { close(); first_word(n); open = true; ++n_rec; }
            else if (!(starts_line && n && line[0] == ';') && open) bases.append(line.data(), n);
            else if (starts_line && n && line[0] != ';' && !open) { gzclose(f); usage_error(path + ": sequence data before the first '>' header"); }
        }
    }
    int zerr = Z_OK; const char* zmsg = gzerror(f, &zerr);
    if (zerr != Z_OK && zerr != Z_STREAM_END) { const std::string m = zmsg ? zmsg : "read error"; gzclose(f); usage_error(path + ": " + m); }
    gzclose(f);
    close();
}
int query_mode(const Options& o, const std::string& prefix, int threads) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t0 = clk::now();
    const std::string fa = prefix + ".unitigs.fa", tsv = prefix + ".query.tsv";
    UnitigFile F; read_unitig_file(o, fa, threads, "-query", F);
    cdbg_ctx* ctx = load_unitig_file(o, fa, F);
    struct Guard { cdbg_ctx* c; ~Guard() { cdbg_destroy(c); } } guard{ ctx };
    F.seq.reset(); F.slices.clear(); F.mp.reset();                 // (the set is resident: the host copy is not needed again)
    const auto t1 = clk::now();
    check(cdbg_index(ctx));
    const auto t2 = clk::now();
    // written beside the target and renamed over it: a failure leaves an earlier table as it was
    struct TmpOut {
        std::string name; FILE* f = nullptr;
        ~TmpOut() { if (f) fclose(f); if (!name.empty()) remove(name.c_str()); }
    } tmp;
    tmp.name = tsv + ".tmp" + std::to_string((long)getpid());
    tmp.f = fopen(tmp.name.c_str(), "w");
    if (!tmp.f) { const std::string n = tmp.name; tmp.name.clear(); usage_error("cannot write " + n); }
    const uint64_t BATCH = 64ull << 20, K = (uint64_t)o.k;
    std::string bases, out; std::vector<std::string> names; std::vector<uint64_t> off{ 0 }, hits;
    uint64_t n_seqs = 0, n_kmers = 0, n_found = 0; double query_s = 0; bool wfail = false;
    auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
    auto flush = [&]() {
        if (names.empty()) return;
        hits.resize(std::max<size_t>(bases.size(), 1));
        const auto q0 = clk::now();
        check(cdbg_query(ctx, bases.data(), off.data(), names.size(), hits.data()));
        query_s += secs(q0, clk::now());
        out.clear();
        for (size_t i = 0; i < names.size(); ++i) {
            const uint64_t b = off[i], len = off[i + 1] - b, nk = len >= K ? len - K + 1 : 0;
            uint64_t found = 0, runs = 0;
            const size_t head = out.size();
            std::string rs;
            uint64_t r_q = 0, r_len = 0, r_u = 0, r_o = 0, r_s = 0, last_o = 0;
            auto close_run = [&]() {
                if (!r_len) return;
                if (runs++) rs.push_back(',');
                put_u(rs, r_q); rs.push_back(':'); put_u(rs, r_len); rs.push_back(':'); put_u(rs, r_u); rs.push_back(':'); rs.push_back(r_s ? '-' : '+'); rs.push_back(':'); put_u(rs, r_o);
                r_len = 0;
            };
            for (uint64_t p = 0; p < nk; ++p) {
                const uint64_t h = hits[b + p];
                if (h == ~0ull) { close_run(); continue; }
                ++found;
                const uint64_t u = h >> 33, uo = (h >> 1) & 0xFFFFFFFFull, st = h & 1;
                if (r_len && u == r_u && st == r_s && uo == (st ? last_o - 1 : last_o + 1)) { ++r_len; last_o = uo; continue; }
                close_run();
                r_q = p; r_len = 1; r_u = u; r_o = uo; r_s = st; last_o = uo;
            }
            close_run();
            (void)head;
            out.append(names[i]); out.push_back('\t'); put_u(out, nk); out.push_back('\t'); put_u(out, found); out.push_back('\t');
            if (runs) out.append(rs); else out.push_back('*');
            out.push_back('\n');
            n_kmers += nk; n_found += found;
        }
        if (fwrite(out.data(), 1, out.size(), tmp.f) != out.size()) wfail = true;
        n_seqs += names.size();
        names.clear(); bases.clear(); off.assign(1, 0);
    };
    parse_queries(o.query, bases, [&](const std::string& name) {
        if (bases.size() > BATCH && !names.empty()) {              // this record would pass 64 MB of bases: what came before it goes first
            const std::string last = bases.substr(off.back());
            bases.resize(off.back());
            flush();
            bases = last;
        }
        names.push_back(name); off.push_back(bases.size());
    });
    flush();
    { FILE* g = tmp.f; tmp.f = nullptr; if (fclose(g) != 0) wfail = true; }
    if (wfail) usage_error("write error on " + tmp.name);
    if (rename(tmp.name.c_str(), tsv.c_str()) != 0) usage_error("cannot rename " + tmp.name + " to " + tsv);
    tmp.name.clear();
    printf("query: %llu sequences, %llu k-mers, %llu found (load %.2f s, index %.2f s, query %.2f s)\n", (unsigned long long)n_seqs,
           (unsigned long long)n_kmers, (unsigned long long)n_found, secs(t0, t1), secs(t1, t2), query_s);
    printf("hits written to %s\n", tsv.c_str());
    return EXIT_SUCCESS;
}

// ---- -thread: the walk of every query sequence through the unitigs, folded into runs on the device (cdbg_load_unitigs + cdbg_index + cdbg_thread + cdbg_fetch_runs) ----
int thread_mode(const Options& o, const std::string& prefix, int threads) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t0 = clk::now();
    const std::string fa = prefix + ".unitigs.fa", tsv = prefix + ".thread.tsv";
    UnitigFile F; read_unitig_file(o, fa, threads, "-thread", F);
    cdbg_ctx* ctx = load_unitig_file(o, fa, F);
    struct Guard { cdbg_ctx* c; ~Guard() { cdbg_destroy(c); } } guard{ ctx };
    F.seq.reset(); F.slices.clear(); F.mp.reset();                 // (the set is resident: the host copy is not needed again)
    const auto t1 = clk::now();
    check(cdbg_index(ctx));
    const auto t2 = clk::now();
    // written beside the target and renamed over it: a failure leaves an earlier table as it was
    struct TmpOut {
        std::string name; FILE* f = nullptr;
        ~TmpOut() { if (f) fclose(f); if (!name.empty()) remove(name.c_str()); }
    } tmp;
    tmp.name = tsv + ".tmp" + std::to_string((long)getpid());
    tmp.f = fopen(tmp.name.c_str(), "w");
    if (!tmp.f) { const std::string n = tmp.name; tmp.name.clear(); usage_error("cannot write " + n); }
    const uint64_t BATCH = 64ull << 20, K = (uint64_t)o.k;
    std::string bases, out; std::vector<std::string> names; std::vector<uint64_t> off{ 0 }, run_off, start, place; std::vector<uint32_t> len;
    uint64_t n_seqs = 0, n_kmers = 0, n_found = 0, n_runs = 0, n_ext = 0; double thread_s = 0; bool wfail = false;
    auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
    auto flush = [&]() {
        if (names.empty()) return;
        uint64_t tot[4];
        const auto q0 = clk::now();
        check(cdbg_thread(ctx, bases.data(), off.data(), names.size(), tot));
        run_off.resize(names.size() + 1); start.resize(std::max<uint64_t>(tot[2], 1)); place.resize(start.size()); len.resize(start.size());
        check(cdbg_fetch_runs(ctx, run_off.data(), start.data(), place.data(), len.data()));
        thread_s += secs(q0, clk::now());
        out.clear();
        for (size_t i = 0; i < names.size(); ++i) {
            const uint64_t b = off[i], n = off[i + 1] - b, nk = n >= K ? n - K + 1 : 0;
            uint64_t found = 0;
            for (uint64_t r = run_off[i]; r < run_off[i + 1]; ++r) found += len[r];
            out.append(names[i]); out.push_back('\t'); put_u(out, nk); out.push_back('\t'); put_u(out, found); out.push_back('\t');
            for (uint64_t r = run_off[i]; r < run_off[i + 1]; ++r) {
                if (r > run_off[i]) out.push_back(',');
                put_u(out, start[r] - b); out.push_back(':'); put_u(out, len[r]); out.push_back(':'); put_u(out, place[r] >> 33); out.push_back(':');
                out.push_back((place[r] & 1) ? '-' : '+'); out.push_back(':'); put_u(out, (place[r] >> 1) & 0xFFFFFFFFull);
            }
            if (run_off[i] == run_off[i + 1]) out.push_back('*');
            out.push_back('\n');
            n_kmers += nk;
        }
        if (fwrite(out.data(), 1, out.size(), tmp.f) != out.size()) wfail = true;
        n_seqs += names.size(); n_found += tot[1]; n_runs += tot[2]; n_ext += tot[3];
        names.clear(); bases.clear(); off.assign(1, 0);
    };
    parse_queries(o.thread, bases, [&](const std::string& name) {
        if (bases.size() > BATCH && !names.empty()) {              // this record would pass 64 MB of bases: what came before it goes first
            const std::string last = bases.substr(off.back());
            bases.resize(off.back());
            flush();
            bases = last;
        }
        names.push_back(name); off.push_back(bases.size());
    });
    flush();
    { FILE* g = tmp.f; tmp.f = nullptr; if (fclose(g) != 0) wfail = true; }
    if (wfail) usage_error("write error on " + tmp.name);
    if (rename(tmp.name.c_str(), tsv.c_str()) != 0) usage_error("cannot rename " + tmp.name + " to " + tsv);
    tmp.name.clear();
    printf("thread: %llu sequences, %llu k-mers, %llu found, %llu runs, %llu extended (load %.2f s, index %.2f s, thread %.2f s)\n", (unsigned long long)n_seqs,
           (unsigned long long)n_kmers, (unsigned long long)n_found, (unsigned long long)n_runs, (unsigned long long)n_ext, secs(t0, t1), secs(t1, t2), thread_s);
    printf("runs written to %s\n", tsv.c_str());
    return EXIT_SUCCESS;
}

// ---- -components: the connected components of the records' graph (cdbg_load_unitigs + cdbg_components + cdbg_fetch_components) ----
int components_mode(const Options& o, const std::string& prefix, int threads) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t0 = clk::now();
    const std::string fa = prefix + ".unitigs.fa", ctsv = prefix + ".components.tsv", utsv = prefix + ".unitig_components.tsv";
    UnitigFile F; read_unitig_file(o, fa, threads, "-components", F);
    const uint64_t nu = F.nu;
    std::vector<uint64_t> kc(nu ? nu : 1, 0);                      // the KC:i: token of every header (0 where a record has none)
    for (uint64_t i = 0; i < nu; ++i) {
        const std::string& r = *F.rest[i];
        for (size_t p = 0; p < r.size();) {
            size_t q = r.find(' ', p); if (q == std::string::npos) q = r.size();
            if (r.compare(p, 5, "KC:i:") == 0) { kc[i] = strtoull(r.c_str() + p + 5, nullptr, 10); break; }
            p = q + 1;
        }
    }
    cdbg_ctx* ctx = load_unitig_file(o, fa, F, kc.data());
    struct Guard { cdbg_ctx* c; ~Guard() { cdbg_destroy(c); } } guard{ ctx };
    F.seq.reset(); F.slices.clear(); F.mp.reset();                 // (the set is resident: the host copy is not needed again)
    const auto t1 = clk::now();
    uint64_t tot[4]; check(cdbg_components(ctx, tot));
    const uint64_t nc = tot[0];
    std::vector<uint32_t> comp(nu ? nu : 1), first(nc ? nc : 1); std::vector<uint64_t> n_un(nc ? nc : 1), bases(n_un.size()), kmers(n_un.size()), ckc(n_un.size());
    check(cdbg_fetch_components(ctx, comp.data(), 0, nc, first.data(), n_un.data(), bases.data(), kmers.data(), ckc.data()));
    const auto t2 = clk::now();
    // both tables are written beside their targets and renamed over them: a failure leaves earlier tables as they were
    struct TmpOut {
        std::string name; FILE* f = nullptr;
        ~TmpOut() { if (f) fclose(f); if (!name.empty()) remove(name.c_str()); }
        void open(const std::string& n) { f = fopen(n.c_str(), "w"); if (!f) usage_error("cannot write " + n); name = n; }
        bool close() { FILE* g = f; f = nullptr; return !g || fclose(g) == 0; }
        bool commit(const std::string& to) { if (rename(name.c_str(), to.c_str()) != 0) return false; name.clear(); return true; }
    } tc, tu;
    tc.open(ctsv + ".tmp" + std::to_string((long)getpid())); tu.open(utsv + ".tmp" + std::to_string((long)getpid()));
    auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
    bool wfail = false; std::string out;
    auto flush = [&](FILE* f, bool all) { if (all || out.size() > (1u << 20)) { if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size()) wfail = true; out.clear(); } };
    out = "#component\tunitigs\tbases\tkmers\tKC\tfirst_unitig\n";
    for (uint64_t c = 0; c < nc; ++c) {
        put_u(out, c); out.push_back('\t'); put_u(out, n_un[c]); out.push_back('\t'); put_u(out, bases[c]); out.push_back('\t'); put_u(out, kmers[c]); out.push_back('\t');
        put_u(out, ckc[c]); out.push_back('\t'); put_u(out, first[c]); out.push_back('\n');
        flush(tc.f, false);
    }
    flush(tc.f, true);
    out = "#unitig\tcomponent\n";
    for (uint64_t u = 0; u < nu; ++u) { put_u(out, u); out.push_back('\t'); put_u(out, comp[u]); out.push_back('\n'); flush(tu.f, false); }
    flush(tu.f, true);
    if (!tc.close()) wfail = true;
    if (!tu.close()) wfail = true;
    if (wfail) usage_error("write error on " + tc.name + " / " + tu.name);
    if (!tc.commit(ctsv)) usage_error("cannot rename " + tc.name + " to " + ctsv);
    if (!tu.commit(utsv)) usage_error("cannot rename " + tu.name + " to " + utsv);
    if (o.verbose) printf("components: %llu components, %llu unitigs in the largest (component %llu), %llu components of one unitig\n", (unsigned long long)tot[0],
                          (unsigned long long)tot[1], (unsigned long long)tot[2], (unsigned long long)tot[3]);
    printf("components: %llu unitigs in %llu components (load %.2f s, components %.2f s)\n", (unsigned long long)nu, (unsigned long long)nc, secs(t0, t1), secs(t1, t2));
    printf("components written to %s and %s\n", ctsv.c_str(), utsv.c_str());
    return EXIT_SUCCESS;
}

// ---- -colors: the unitigs coloured by sample (cdbg_load_unitigs + cdbg_color_open + cdbg_color per sample + cdbg_color_classes + the two fetches) ----
int colors_mode(const Options& o, const std::string& prefix, int threads) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t0 = clk::now();
    // the list first: line i names the sample of colour i (empty lines are skipped); every sample must be readable before anything is loaded
    std::vector<std::string> samples;
    {
        std::ifstream lf(o.colors);
        if (!lf) usage_error("cannot open sample list " + o.colors);
        std::string line;
        while (std::getline(lf, line)) {
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
            if (!line.empty()) samples.push_back(line);
        }
    }
    if (samples.empty()) usage_error("-colors: no samples in " + o.colors);
    if (samples.size() > CDBG_MAX_COLORS) usage_error("-colors: " + std::to_string(samples.size()) + " samples in " + o.colors + ", at most " + std::to_string(CDBG_MAX_COLORS) + " (CDBG_MAX_COLORS)");
    for (const std::string& sf : samples) { FILE* f = fopen(sf.c_str(), "rb"); if (!f) usage_error("cannot open sample file " + sf); fclose(f); }
    if (!o.color_query.empty()) { FILE* f = fopen(o.color_query.c_str(), "rb"); if (!f) usage_error("cannot open query file " + o.color_query); fclose(f); }
    const std::string fa = prefix + ".unitigs.fa", rtsv = prefix + ".colors.tsv", ctsv = prefix + ".color_classes.tsv", qtsv = prefix + ".color_query.tsv";
    UnitigFile F; read_unitig_file(o, fa, threads, "-colors", F);
    cdbg_ctx* ctx = load_unitig_file(o, fa, F);
    struct Guard { cdbg_ctx* c; ~Guard() { cdbg_destroy(c); } } guard{ ctx };
    const uint64_t nu = F.nu;
    F.seq.reset(); F.slices.clear(); F.mp.reset();                 // (the set is resident: the host copy is not needed again)
    const auto t1 = clk::now();
    const uint32_t N = (uint32_t)samples.size();
    check(cdbg_color_open(ctx, N));
    const auto t2 = clk::now();
    const uint64_t BATCH = 64ull << 20;
    uint64_t tot[3] = { 0, 0, 0 };
    for (uint32_t col = 0; col < N; ++col) {
        std::string bases; std::vector<uint64_t> off{ 0 };
        auto flush = [&]() {
            if (off.size() == 1) return;
            uint64_t out[3];
            check(cdbg_color(ctx, col, bases.data(), off.data(), off.size() - 1, out));
            for (int i = 0; i < 3; ++i) tot[i] += out[i];
            bases.clear(); off.assign(1, 0);
        };
        parse_queries(samples[col], bases, [&](const std::string&) {
            if (bases.size() > BATCH && off.size() > 1) {              // this record would pass 64 MB of bases: what came before it goes first
                const std::string last = bases.substr(off.back());
                bases.resize(off.back());
                flush();
                bases = last;
            }
            off.push_back(bases.size());
        }, "sample file");
        flush();
    }
    const auto t3 = clk::now();
    uint64_t info[4]; check(cdbg_color_classes(ctx, info));
    const uint64_t R = info[0], NC = info[1], NW = (N + 31) / 32;
    std::vector<uint64_t> run_off(nu + 1), c_runs(NC ? NC : 1), c_kmers(NC ? NC : 1);
    std::vector<uint32_t> r_off(R ? R : 1), r_len(R ? R : 1), r_cls(R ? R : 1), c_ncol(NC ? NC : 1), c_bits(NC ? NC * NW : 1);
    check(cdbg_fetch_color_runs(ctx, run_off.data(), r_off.data(), r_len.data(), r_cls.data()));
    check(cdbg_fetch_color_classes(ctx, 0, NC, c_ncol.data(), c_runs.data(), c_kmers.data(), c_bits.data()));
    const auto t4 = clk::now();
    // both tables are written beside their targets and renamed over them: a failure leaves earlier tables as they were
    struct TmpOut {
        std::string name; FILE* f = nullptr;
        ~TmpOut() { if (f) fclose(f); if (!name.empty()) remove(name.c_str()); }
        void open(const std::string& n) { f = fopen(n.c_str(), "w"); if (!f) usage_error("cannot write " + n); name = n; }
        bool close() { FILE* g = f; f = nullptr; return !g || fclose(g) == 0; }
        bool commit(const std::string& to) { if (rename(name.c_str(), to.c_str()) != 0) return false; name.clear(); return true; }
    } tr, tc, tq;
    tr.open(rtsv + ".tmp" + std::to_string((long)getpid())); tc.open(ctsv + ".tmp" + std::to_string((long)getpid()));
    auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
    bool wfail = false; std::string out;
    auto flush_out = [&](FILE* f, bool all) { if (all || out.size() > (1u << 20)) { if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size()) wfail = true; out.clear(); } };
    for (uint64_t u = 0; u < nu; ++u)
        for (uint64_t r = run_off[u]; r < run_off[u + 1]; ++r) {
            put_u(out, u); out.push_back('\t'); put_u(out, r_off[r]); out.push_back('\t'); put_u(out, r_len[r]); out.push_back('\t'); put_u(out, r_cls[r]); out.push_back('\n');
            flush_out(tr.f, false);
        }
    flush_out(tr.f, true);
    for (uint64_t c = 0; c < NC; ++c) {
        put_u(out, c); out.push_back('\t'); put_u(out, c_ncol[c]); out.push_back('\t'); put_u(out, c_runs[c]); out.push_back('\t'); put_u(out, c_kmers[c]); out.push_back('\t');
        bool first = true;
        for (uint32_t col = 0; col < N; ++col)
            if ((c_bits[c * NW + (col >> 5)] >> (col & 31)) & 1u) { if (!first) out.push_back(','); put_u(out, col); first = false; }
        if (first) out.push_back('-');
        out.push_back('\n');
        flush_out(tc.f, false);
    }
    flush_out(tc.f, true);
    if (!tr.close()) wfail = true;
    if (!tc.close()) wfail = true;
    if (wfail) usage_error("write error on " + tr.name + " / " + tc.name);
    if (!tr.commit(rtsv)) usage_error("cannot rename " + tr.name + " to " + rtsv);
    if (!tc.commit(ctsv)) usage_error("cannot rename " + tc.name + " to " + ctsv);
    if (o.verbose) printf("colors: %llu positions with a colour, %llu unitigs that are one run, %llu k-mers extended\n", (unsigned long long)info[2], (unsigned long long)info[3], (unsigned long long)tot[2]);
    printf("colors: %u samples, %llu k-mers, %llu found, %llu runs, %llu classes (load %.2f s, index %.2f s, mark %.2f s, classes %.2f s)\n", N, (unsigned long long)tot[0],
           (unsigned long long)tot[1], (unsigned long long)R, (unsigned long long)NC, secs(t0, t1), secs(t1, t2), secs(t2, t3), secs(t3, t4));
    printf("colours written to %s and %s\n", rtsv.c_str(), ctsv.c_str());
    if (o.color_query.empty()) return EXIT_SUCCESS;
    // -color-query: name, windows, found, colours reported, their indices ('*' for none) per sequence, in batches of 64 MB of bases
    tq.open(qtsv + ".tmp" + std::to_string((long)getpid()));
    const uint64_t K = (uint64_t)o.k;
    std::string bases; std::vector<std::string> names; std::vector<uint64_t> off{ 0 }; std::vector<uint32_t> q_found, q_ncol, q_bits;
    uint64_t n_seqs = 0, n_kmers = 0, n_found = 0, n_segs = 0, n_rep = 0; double query_s = 0;
    auto flush = [&]() {
        if (names.empty()) return;
        uint64_t qt[5];
        const auto q0 = clk::now();
        check(cdbg_color_query(ctx, bases.data(), off.data(), names.size(), o.share_num, o.share_den, o.share_of_found ? 1 : 0, qt));
        q_found.resize(names.size()); q_ncol.resize(names.size()); q_bits.resize(names.size() * NW);
        check(cdbg_fetch_color_query(ctx, q_found.data(), q_ncol.data(), q_bits.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
        query_s += secs(q0, clk::now());
        out.clear();
        for (size_t i = 0; i < names.size(); ++i) {
            const uint64_t n = off[i + 1] - off[i], nk = n >= K ? n - K + 1 : 0;
            out.append(names[i]); out.push_back('\t'); put_u(out, nk); out.push_back('\t'); put_u(out, q_found[i]); out.push_back('\t'); put_u(out, q_ncol[i]); out.push_back('\t');
            bool first = true;
            for (uint32_t col = 0; col < N; ++col)
                if ((q_bits[i * NW + (col >> 5)] >> (col & 31)) & 1u) { if (!first) out.push_back(','); put_u(out, col); first = false; }
            if (first) out.push_back('*');
            out.push_back('\n');
            n_kmers += nk;
        }
        flush_out(tq.f, true);
        n_seqs += names.size(); n_found += qt[1]; n_segs += qt[2]; n_rep += qt[3];
        names.clear(); bases.clear(); off.assign(1, 0);
    };
    parse_queries(o.color_query, bases, [&](const std::string& name) {
        if (bases.size() > BATCH && !names.empty()) {              // this record would pass 64 MB of bases: what came before it goes first
            const std::string last = bases.substr(off.back());
            bases.resize(off.back());
            flush();
            bases = last;
        }
        names.push_back(name); off.push_back(bases.size());
    });
    flush();
    if (!tq.close()) wfail = true;
    if (wfail) usage_error("write error on " + tq.name);
    if (!tq.commit(qtsv)) usage_error("cannot rename " + tq.name + " to " + qtsv);
    printf("color-query: %llu sequences, %llu k-mers, %llu found, %llu segments, %llu sequences with a colour, share %u/%u of %s (query %.2f s)\n", (unsigned long long)n_seqs,
           (unsigned long long)n_kmers, (unsigned long long)n_found, (unsigned long long)n_segs, (unsigned long long)n_rep, o.share_num, o.share_den,
           o.share_of_found ? "the k-mers found" : "all k-mers", query_s);
    printf("colour query written to %s\n", qtsv.c_str());
    return EXIT_SUCCESS;
}

// ---- -quantify: the k-mers of a sample counted per unitig (cdbg_load_unitigs + cdbg_quantify + cdbg_fetch_quant) ----
int quantify_mode(const Options& o, const std::string& prefix, int threads) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t0 = clk::now();
    const std::string fa = prefix + ".unitigs.fa", tsv = prefix + ".quant.tsv";
    UnitigFile F; read_unitig_file(o, fa, threads, "-quantify", F);
    cdbg_ctx* ctx = load_unitig_file(o, fa, F);
    struct Guard { cdbg_ctx* c; ~Guard() { cdbg_destroy(c); } } guard{ ctx };
    const uint64_t nu = F.nu, K = (uint64_t)o.k;
    std::vector<uint64_t> nk(nu ? nu : 1);                         // k-mer positions per unitig, file order
    uint64_t n_pos = 0;
    for (uint64_t i = 0; i < nu; ++i) { nk[i] = F.off[i + 1] - F.off[i] - K + 1; n_pos += nk[i]; }
    F.seq.reset(); F.slices.clear(); F.mp.reset();                 // (the set is resident: the host copy is not needed again)
    const auto t1 = clk::now();
    check(cdbg_index(ctx));
    const auto t2 = clk::now();
    // written beside the target and renamed over it: a failure leaves an earlier table as it was
    struct TmpOut {
        std::string name; FILE* f = nullptr;
        ~TmpOut() { if (f) fclose(f); if (!name.empty()) remove(name.c_str()); }
    } tmp;
    tmp.name = tsv + ".tmp" + std::to_string((long)getpid());
    tmp.f = fopen(tmp.name.c_str(), "w");
    if (!tmp.f) { const std::string n = tmp.name; tmp.name.clear(); usage_error("cannot write " + n); }
    const uint64_t BATCH = 64ull << 20;
    std::string bases; std::vector<uint64_t> off{ 0 };
    uint64_t n_seqs = 0, tot[3] = { 0, 0, 0 }; double quant_s = 0;
    auto flush = [&]() {
        if (off.size() == 1) return;
        uint64_t out[3];
        const auto q0 = clk::now();
        check(cdbg_quantify(ctx, bases.data(), off.data(), off.size() - 1, out));
        quant_s += secs(q0, clk::now());
        for (int i = 0; i < 3; ++i) tot[i] += out[i];
        n_seqs += off.size() - 1;
        bases.clear(); off.assign(1, 0);
    };
    parse_queries(o.quantify, bases, [&](const std::string&) {
        if (bases.size() > BATCH && off.size() > 1) {              // this record would pass 64 MB of bases: what came before it goes first
            const std::string last = bases.substr(off.back());
            bases.resize(off.back());
            flush();
            bases = last;
        }
        off.push_back(bases.size());
    }, "sample file");
    flush();
    if (!n_seqs) { uint64_t out[3]; const uint64_t z[1] = { 0 }; check(cdbg_quantify(ctx, "", z, 0, out)); }
    std::vector<uint64_t> kc(nu ? nu : 1), aboff(nu + 1); std::vector<uint32_t> cov(nu ? nu : 1), ab(o.all_ab ? n_pos + 1 : 1);
    const auto f0 = clk::now();
    check(cdbg_fetch_quant(ctx, 0, nu, kc.data(), cov.data(), o.all_ab ? ab.data() : nullptr, o.all_ab ? aboff.data() : nullptr));
    quant_s += secs(f0, clk::now());
    auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
    bool wfail = false; std::string out;
    for (uint64_t i = 0; i < nu; ++i) {
        put_u(out, i); out.push_back('\t'); put_u(out, nk[i]); out.push_back('\t'); put_u(out, kc[i]); out.push_back('\t'); put_u(out, cov[i]); out.push_back('\t');
        put_km(out, (double)kc[i] / (double)nk[i]);
        if (o.all_ab) {
            out.push_back('\t');
            for (uint64_t j = aboff[i]; j < aboff[i + 1]; ++j) { if (j > aboff[i]) out.push_back(','); put_u(out, ab[j]); }
        }
        out.push_back('\n');
        if (out.size() > (1u << 22) || i + 1 == nu) { if (fwrite(out.data(), 1, out.size(), tmp.f) != out.size()) wfail = true; out.clear(); }
    }
    { FILE* g = tmp.f; tmp.f = nullptr; if (fclose(g) != 0) wfail = true; }
    if (wfail) usage_error("write error on " + tmp.name);
    if (rename(tmp.name.c_str(), tsv.c_str()) != 0) usage_error("cannot rename " + tmp.name + " to " + tsv);
    tmp.name.clear();
    printf("quantify: %llu sequences, %llu k-mers, %llu found, %llu extended (load %.2f s, index %.2f s, quantify %.2f s)\n", (unsigned long long)n_seqs,
           (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2], secs(t0, t1), secs(t1, t2), quant_s);
    printf("counts written to %s\n", tsv.c_str());
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && (!strcmp(argv[1], "-version") || !strcmp(argv[1], "-v"))) {
        printf("BCALM 2 CLI, MI355X-native engine, version %s\nUsing libcdbg (HIP, gfx950) instead of gatb-core\n", CDBG_VERSION);
        return EXIT_SUCCESS;
    }
    try {
        Options o = parse(argc, argv);
        printf("BCALM 2 CLI, MI355X-native engine, version %s\n", CDBG_VERSION);
        if (o.in.empty()) usage_error("Specifiy -in");             // sic: the reference's message (bcalm_1.cpp:61)
        std::string prefix = o.out.empty() ? base_name(o.in) : o.out;
        if ((o.skip_bcalm || o.skip_bglue) && !o.redo_links) usage_error("-skip-bcalm and -skip-bglue are only supported together with -redo-links (no glue files are kept between runs)");
        if (!o.colors.empty() && (o.components || !o.thread.empty() || !o.query.empty() || !o.quantify.empty() || o.redo_links)) usage_error("-colors, -components, -thread, -query, -quantify and -redo-links are separate modes: give one of them");
        if (!o.color_query.empty() && o.colors.empty()) usage_error("-color-query needs -colors <list>: the samples whose colours the sequences are asked for");
        if (!o.colors.empty() && o.n_gpus != 1) usage_error("-colors runs on one GPU: -nb-gpus must be 1");
        if (o.components && (!o.thread.empty() || !o.query.empty() || !o.quantify.empty() || o.redo_links)) usage_error("-components, -thread, -query, -quantify and -redo-links are separate modes: give one of them");
        if (o.components && o.n_gpus != 1) usage_error("-components runs on one GPU: -nb-gpus must be 1");
        if (!o.thread.empty() && (!o.query.empty() || !o.quantify.empty() || o.redo_links)) usage_error("-thread, -query, -quantify and -redo-links are separate modes: give one of them");
        if (!o.thread.empty() && o.n_gpus != 1) usage_error("-thread runs on one GPU: -nb-gpus must be 1");
        if (!o.quantify.empty() && (!o.query.empty() || o.redo_links)) usage_error("-quantify, -query and -redo-links are separate modes: give one of them");
        if (!o.quantify.empty() && o.n_gpus != 1) usage_error("-quantify runs on one GPU: -nb-gpus must be 1");
        if (!o.query.empty() && o.redo_links) usage_error("-query and -redo-links are two modes: give one of them");
        if (!o.query.empty() && o.n_gpus != 1) usage_error("-query runs on one GPU: -nb-gpus must be 1");
        if (o.redo_links || !o.query.empty() || !o.quantify.empty() || !o.thread.empty() || o.components || !o.colors.empty()) {
            if (o.n_gpus != 1) usage_error("-redo-links runs on one GPU: -nb-gpus must be 1");
            const std::string suffix = ".unitigs.fa";                // -in may name the unitigs file itself, or the input (even the deleted .h5) of the run that wrote it
            if (o.out.empty() && o.in.size() > suffix.size() && o.in.compare(o.in.size() - suffix.size(), suffix.size(), suffix) == 0) {
                const size_t sl = o.in.find_last_of('/');
                prefix = o.in.substr(sl == std::string::npos ? 0 : sl + 1); prefix.resize(prefix.size() - suffix.size());
            }
            int threads = o.cores > 0 ? o.cores : (int)std::min<unsigned>(usable_cpus(), 32u);
            if (!o.colors.empty()) return colors_mode(o, prefix, std::max(1, std::min(threads, 60)));
            if (o.components) return components_mode(o, prefix, std::max(1, std::min(threads, 60)));
            if (!o.thread.empty()) return thread_mode(o, prefix, std::max(1, std::min(threads, 60)));
            if (!o.quantify.empty()) return quantify_mode(o, prefix, std::max(1, std::min(threads, 60)));
            if (!o.query.empty()) return query_mode(o, prefix, std::max(1, std::min(threads, 60)));
            return redo_links(o, prefix, std::max(1, std::min(threads, 60)));
        }
        auto t0 = std::chrono::steady_clock::now();

        if (o.n_gpus < 1 || (o.n_gpus & (o.n_gpus - 1))) usage_error("-nb-gpus must be a power of two");
        const int world = o.n_gpus;
        // one context per GPU; with several GPUs the reads are sharded over them and the contexts talk over RCCL inside
        // libcdbg (include/cdbg.h "Multi-GPU"); every rank ends with its SHARE of the unitigs, links the whole set collectively (job-wide ids)
        // and its share is written from its own context -- round 4 gathered the whole graph on every rank (emit_replicated) for rank 0 to write
        std::vector<cdbg_ctx*> ctxs(world, nullptr);
        cdbg_ctx* ctx = nullptr;
        auto make_contexts = [&]() {
            for (int r = 0; r < world; ++r) {
                cdbg_params p{}; p.k = o.k; p.abundance_min = o.amin; p.minimizer_size = o.m; p.log2_partitions = o.log_np;
                p.device_id = world > 1 ? r : o.device; p.world_size = world; p.rank = r; p.all_abundance_counts = o.all_ab ? 1 : 0;
                p.emit_replicated = 0;
                check(cdbg_create(&p, &ctxs[r]));
            }
            ctx = ctxs[0];
            // (CDBG_FORCE_MULTI, the library's test hook: one rank through the multi-rank code path -- it needs the transport then)
            if (world > 1 || getenv("CDBG_FORCE_MULTI")) {
                unsigned char uid[128]; check(cdbg_comm_unique_id(uid));
                std::vector<std::thread> th; std::atomic<int> bad{0}; std::vector<std::string> errs(world);
                for (int r = 0; r < world; ++r) th.emplace_back([&, r]() { if (cdbg_comm_init_rccl(ctxs[r], uid) != 0) { errs[r] = cdbg_last_error(); ++bad; } });
                for (auto& t : th) t.join();
                if (bad) for (auto& e : errs) if (!e.empty()) usage_error(e);
            }
        };
        make_contexts();
        auto t_init = std::chrono::steady_clock::now();
        int threads = o.cores > 0 ? o.cores : (int)std::min<unsigned>(usable_cpus(), 32u);
        threads = std::max(1, std::min(threads, 60));        // (each parser thread holds one of the library's 64 staging buffers)
        std::vector<std::string> files;
        if (looks_like_file_list(o.in)) {
            gzFile f = gzopen(o.in.c_str(), "rb"); char buf[4096];
            while (gzgets(f, buf, sizeof buf)) { size_t n = strlen(buf); while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) buf[--n] = 0; if (n) files.push_back(buf); }
            gzclose(f);
        } else files.push_back(o.in);
        uint64_t n_seq = 0, n_bases = 0;
        for (int attempt = 0;; ++attempt) {
            if (world == 1 && !o.no_stream) {                // announce the volume: the scan starts while the input is still being parsed
                uint64_t est = 0; for (const auto& f : files) est += estimate_text_bytes(f);
                if (est) check(cdbg_expect_input(ctx, est));
            }
            Ingest I; I.ctxs = ctxs; I.k = o.k;
            const bool regular = ingest_files(I, files, threads, attempt == 0);
            n_seq = I.n_seq; n_bases = I.n_bases;
            if (regular) break;
            // a FASTQ file whose records are not all four lines: start over with the tolerant serial parser
            for (int r = 0; r < world; ++r) { cdbg_destroy(ctxs[r]); ctxs[r] = nullptr; }
            make_contexts();
        }
        auto t1 = std::chrono::steady_clock::now();
        // the stages are collective: one host thread per GPU
        auto all_ranks = [&](int (*stage)(cdbg_ctx*)) {
            if (world == 1) { check(stage(ctx)); return; }
            std::vector<std::thread> th; std::atomic<int> bad{0}; std::vector<std::string> errs(world);
            for (int r = 0; r < world; ++r) th.emplace_back([&, r]() { if (stage(ctxs[r]) != 0) { errs[r] = cdbg_last_error(); ++bad; } });
            for (auto& t : th) t.join();
            if (bad) for (auto& e : errs) if (!e.empty()) throw std::runtime_error(e);
        };
        all_ranks(cdbg_count);
        if (!o.solid_out.empty()) {                          // solid k-mer dump: "<canonical k-mer> <abundance>" per line
            FILE* sf = fopen(o.solid_out.c_str(), "w");
            if (!sf) usage_error("cannot write " + o.solid_out);
            for (int r = 0; r < world; ++r) {                // (every rank holds the solid k-mers of its partitions)
                uint64_t ns = 0, got = 0; check(cdbg_num_solid(ctxs[r], &ns));
                std::vector<char> km((ns + 1) * (size_t)(o.k + 1)); std::vector<uint32_t> cnt(ns + 1);
                check(cdbg_fetch_solid(ctxs[r], km.data(), cnt.data(), ns, &got));
                for (uint64_t i = 0; i < got; ++i) fprintf(sf, "%s %u\n", km.data() + i * (size_t)(o.k + 1), cnt[i]);
            }
            fclose(sf);
        }
        all_ranks(cdbg_compact);
        all_ranks(cdbg_glue);
        auto t_stages = std::chrono::steady_clock::now();
        cdbg_stats_t st; check(cdbg_stats(ctx, &st));
        // edges between unitigs (README.md:72 L: tokens; convertToGFA.py:103-112 GFA L lines).  Several GPUs: every rank holds a share of
        // the unitigs; cdbg_link is collective there and numbers the unitigs job-wide, rank after rank (include/cdbg.h)
        all_ranks(cdbg_link);
        for (int r = 1; r < world; ++r) {                    // (the printed totals: k-mers and pieces of every rank's partitions, unitigs of every rank's share)
            cdbg_stats_t sr; check(cdbg_stats(ctxs[r], &sr));
            st.n_occurrences += sr.n_occurrences; st.n_distinct += sr.n_distinct; st.n_solid += sr.n_solid; st.n_pieces += sr.n_pieces;
            st.n_unitigs += sr.n_unitigs; st.unitig_bases += sr.unitig_bases;
            st.ms_count = std::max(st.ms_count, sr.ms_count); st.ms_compact = std::max(st.ms_compact, sr.ms_compact); st.ms_glue = std::max(st.ms_glue, sr.ms_glue);
        }

        // Output: rank after rank (one rank: everything), each rank's share fetched, formatted by the threads in blocks of unitigs (own
        // integer formatting; "%.1f" stays with printf so that km:f: rounds exactly as the reference's) and written in block order, one
        // write per block.  Ids and link targets are job-wide.
        const std::string fa = prefix + ".unitigs.fa";
        FILE* out = fopen(fa.c_str(), "w");
        if (!out) usage_error("cannot write " + fa);
        FILE* gfa = nullptr;
        if (o.gfa) { gfa = fopen((prefix + ".unitigs.gfa").c_str(), "w"); if (gfa) fprintf(gfa, "H\tVN:Z:1.0\tks:i:%d\n", o.k); }
        double s_fetch = 0, s_write = 0;
        for (int r = 0; r < world; ++r) {
        auto tf0 = std::chrono::steady_clock::now();
        cdbg_ctx* const cx = ctxs[r];
        uint64_t nu = 0, tb = 0; check(cdbg_num_unitigs(cx, &nu, &tb));
        uint64_t id0 = 0, id_total = 0; check(cdbg_unitig_id_base(cx, &id0, &id_total));
        std::unique_ptr<char[]> seq(new char[tb + 1]);       // (not value-initialised: a gigabyte at config 3)
        std::vector<uint64_t> off(nu + 1), kc(nu ? nu : 1);
        check(cdbg_fetch_unitigs(cx, 0, nu, seq.get(), off.data(), kc.data()));
        std::vector<uint32_t> ab; std::vector<uint64_t> aboff;
        if (o.all_ab) { ab.resize(tb + 1); aboff.resize(nu + 1); check(cdbg_fetch_unitig_abundances(cx, 0, nu, ab.data(), aboff.data())); }
        uint64_t nl = 0; check(cdbg_num_links(cx, &nl));
        std::vector<uint64_t> loff(2 * nu + 1); std::vector<uint32_t> lto(nl ? nl : 1);
        check(cdbg_fetch_links(cx, loff.data(), lto.data()));
        auto tf1 = std::chrono::steady_clock::now();
        {
            const uint64_t BLOCK = 1u << 15;
            const uint64_t nblocks = (nu + BLOCK - 1) / BLOCK;
            std::atomic<uint64_t> next_block{0};
            std::mutex wm; std::condition_variable wcv; uint64_t turn = 0; bool wfail = false;
            auto put_u = [](std::string& d, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) d.push_back(t[--n]); };
            auto writer = [&]() {
                std::string fb, gb;
                for (;;) {
                    const uint64_t b = next_block.fetch_add(1);
                    if (b >= nblocks) break;
                    fb.clear(); gb.clear();
                    const uint64_t i0 = b * BLOCK, i1 = std::min(nu, i0 + BLOCK);
                    fb.reserve((size_t)(off[i1] - off[i0]) + (size_t)(i1 - i0) * 96);
                    for (uint64_t i = i0; i < i1; ++i) {
                        const uint64_t len = off[i + 1] - off[i], id = id0 + i;
                        const double km = (double)kc[i] / (double)(len - (uint64_t)o.k + 1);
                        fb.push_back('>'); put_u(fb, id); fb.append(" LN:i:"); put_u(fb, len);
                        if (o.all_ab) {                          // ><id> LN:i:<length> ab:Z:<abundance_0> ... (README.md:76)
                            fb.append(" ab:Z:");
                            for (uint64_t j = aboff[i]; j < aboff[i + 1]; ++j) { if (j != aboff[i]) fb.push_back(' '); put_u(fb, ab[j]); }
                        } else { fb.append(" KC:i:"); put_u(fb, kc[i]); fb.append(" km:f:"); put_km(fb, km); }
                        if (gfa) { gb.append("S\t"); put_u(gb, id); gb.push_back('\t'); gb.append(seq.get() + off[i], (size_t)len);
                                   gb.append("\tLN:i:"); put_u(gb, len); gb.append("\tKC:i:"); put_u(gb, kc[i]); gb.append("\tkm:f:"); put_km(gb, km); gb.push_back('\n'); }
                        for (int side = 1; side >= 0; --side)    // '+' links (through the last k-mer) first, then '-'
                            for (uint64_t j = loff[2 * i + side]; j < loff[2 * i + side + 1]; ++j) {
                                const char fs = side ? '+' : '-', ts = (lto[j] & 1u) ? '-' : '+';
                                fb.append(" L:"); fb.push_back(fs); fb.push_back(':'); put_u(fb, lto[j] >> 1); fb.push_back(':'); fb.push_back(ts);
                                if (gfa) { gb.append("L\t"); put_u(gb, id); gb.push_back('\t'); gb.push_back(fs); gb.push_back('\t'); put_u(gb, lto[j] >> 1);
                                           gb.push_back('\t'); gb.push_back(ts); gb.push_back('\t'); put_u(gb, (unsigned long long)(o.k - 1)); gb.append("M\n"); }
                            }
                        fb.append(" \n");
                        fb.append(seq.get() + off[i], (size_t)len); fb.push_back('\n');
                    }
                    std::unique_lock<std::mutex> l(wm);
                    wcv.wait(l, [&] { return turn == b; });
                    if (fwrite(fb.data(), 1, fb.size(), out) != fb.size()) wfail = true;
                    if (gfa && fwrite(gb.data(), 1, gb.size(), gfa) != gb.size()) wfail = true;
                    ++turn; wcv.notify_all();
                }
            };
            const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, nblocks));
            std::vector<std::thread> th;
            for (int i = 1; i < nt; ++i) th.emplace_back(writer);
            writer();
            for (auto& t : th) t.join();
            if (wfail) usage_error("write error on " + fa);
        }
        auto tf2 = std::chrono::steady_clock::now();
        s_fetch += std::chrono::duration<double>(tf1 - tf0).count(); s_write += std::chrono::duration<double>(tf2 - tf1).count();
        }
        fclose(out); if (gfa) fclose(gfa);
        auto t3 = std::chrono::steady_clock::now();
        const auto t2 = t3 - std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(s_write));   // (fetches and writes alternate with several ranks: the printed split is their sums)
        auto sec = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
        printf("input: %llu sequences, %llu bases (%.2f s parse)\n", (unsigned long long)n_seq, (unsigned long long)n_bases, sec(t_init, t1));
        uint64_t in_bytes = 0; for (const auto& f : files) { struct stat sb; if (stat(f.c_str(), &sb) == 0) in_bytes += (uint64_t)sb.st_size; }
        uint64_t out_bytes = 0; { struct stat sb; if (stat(fa.c_str(), &sb) == 0) out_bytes = (uint64_t)sb.st_size; }
        printf("host: init %.2f s; ingest %.2f s = %.2f GB/s of input files (%d threads: parse into pinned buffers + H2D + the overlapped scan); stages %.2f s; links + D2H %.2f s; write %.2f s = %.2f GB/s (%d threads)\n",
               sec(t0, t_init), sec(t_init, t1), (double)in_bytes / 1e9 / std::max(1e-9, sec(t_init, t1)), threads, sec(t1, t_stages), sec(t_stages, t2), sec(t2, t3),
               (double)out_bytes / 1e9 / std::max(1e-9, sec(t2, t3)), threads);
        printf("k-mers: %llu occurrences, %llu distinct, %llu solid (abundance >= %d)\n", (unsigned long long)st.n_occurrences,
               (unsigned long long)st.n_distinct, (unsigned long long)st.n_solid, o.amin);
        printf("graph: %llu pieces -> %llu unitigs, %llu bases; minimizer size %d, 2^%d partitions\n", (unsigned long long)st.n_pieces,
               (unsigned long long)st.n_unitigs, (unsigned long long)st.unitig_bases, st.minimizer_size, st.log2_partitions);
        printf("GPU: scan %.2f+%.2f ms (%llu of %llu tiles scanned while the input was arriving), count %.2f ms, compact %.2f ms, glue %.2f ms; stages+links+D2H %.2f s; write %.2f s; end to end %.2f s\n",
               st.ms_scan_hist, st.ms_scan_emit, (unsigned long long)st.n_tiles_overlapped, (unsigned long long)st.n_launch_scan, st.ms_count, st.ms_compact, st.ms_glue, sec(t1, t2), sec(t2, t3), sec(t0, t3));
        printf("unitigs written to %s\n", fa.c_str());
        for (cdbg_ctx* x : ctxs) cdbg_destroy(x);
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
