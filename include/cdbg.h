/* cdbg.h -- C ABI of libcdbg.so: MI355X-native compacted de Bruijn graph construction.
 *
 * DROP-IN BOUNDARY.  The reference has no FFI: its whole hot path is ONE statically
 * linked C++ call,
 *     GraphUnitigsTemplate<span>::create(IProperties*, false)
 *         /root/reference/src/bcalm_1.cpp:57   (span chosen by Integer::apply, :95)
 * fed by the option parser borrowed at /root/reference/src/bcalm_1.cpp:31 and the three
 * properties the wrapper itself reads: STR_URI_INPUT (:55), STR_URI_OUTPUT (:69-72),
 * STR_KMER_SIZE (:92).  This header is what a binding for that call site binds instead
 * (INTEGRATION.md shows the replacement of bcalm_1.cpp's Functor body and the ctypes
 * stub).  Plain C types only, opaque context, caller-owned host buffers, no C++
 * exception crosses the boundary (the reference maps gatb Exceptions to a message +
 * exit 1 at /root/reference/src/main.cpp:39-48; here: negative return code +
 * cdbg_last_error()).
 *
 * Stage entry points mirror what create() runs internally:
 *   cdbg_count    a4-a6  read scan -> minimizer partitions -> solid (k-mer, count)
 *   cdbg_compact  a7-a8  per-bucket compaction in LDS -> pieces + glue records
 *   cdbg_glue     a9     hash-join on junction (k-1)-mers + list ranking -> unitigs
 * All functions return 0 on success and a negative code on error.
 */
#ifndef CDBG_H
#define CDBG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cdbg_ctx cdbg_ctx;

typedef struct cdbg_params {
    int k;                    /* -kmer-size (README.md:17-19,99): any k in 3..255, even or odd (the reference's KSIZE_LIST "32 64 96 128" and the
                                 larger spans it takes as a build option, README.md:91-99; here: CDBG_MAX_W words of 32 bases, default 8) */
    int abundance_min;        /* -abundance-min (README.md:21-25): keep k-mers seen >= this many times */
    int minimizer_size;       /* -minimizer-size (example/circular_unitigs_unittests/CMD:4); 0 = auto */
    int log2_partitions;      /* minimizer partitions = 1 << this; -1 = auto from the input volume */
    int device_id;            /* HIP device ordinal */
    int world_size;           /* GPUs sharing the minimizer space (power of two); 1 = single GPU */
    int rank;                 /* this context owns partitions p with p % world_size == rank */
    int all_abundance_counts; /* -all-abundance-counts (README.md:74-80): keep the abundance of every k-mer of every unitig */
    int emit_replicated;      /* world_size > 1: 0 = every rank emits the unitigs whose head piece it owns (the union over the
                                 ranks is the graph); 1 = every rank emits the complete set (the CLI's rank 0 writes one file) */
    int reads_replicated;     /* world_size > 1: 0 = every rank holds a SHARD of the reads and the super-k-mer records travel to
                                 the partition owners; 1 = every rank holds ALL the reads and scans them for
                                 its own partitions only -- no record exchange (X0: the better choice on 2-4 GPUs, where one
                                 xGMI link would have to carry a large share of the records; free with cdbg_generate_reads) */
} cdbg_params;

typedef struct cdbg_stats_t {
    uint64_t input_bytes;         /* bytes scanned (bases + separators) */
    uint64_t n_records;           /* super-k-mer records written */
    uint64_t n_member_kmers;      /* k-mer occurrences stored in records (home + traveller copies) */
    uint64_t n_occurrences;       /* k-mer occurrences (home only) */
    uint64_t n_distinct;          /* distinct canonical k-mers (the metric's numerator) */
    uint64_t n_solid;             /* solid k-mers (count >= abundance_min) */
    uint64_t n_solid_travellers;  /* solid traveller copies held next to foreign junctions */
    uint64_t n_pieces;            /* compacted pieces before glue */
    uint64_t n_glue_open_ends;    /* open piece ends posted to the glue table */
    uint64_t n_glue_joined;       /* junctions joined by glue */
    uint64_t n_unitigs;
    uint64_t unitig_bases;
    uint64_t n_big_partitions;    /* partitions that fell back to HBM tables (count + compact) */
    uint64_t n_cycles;            /* circular unitigs cut open (in-bucket + across buckets) */
    int minimizer_size, log2_partitions, kmer_words;
    float ms_scan_hist, ms_scan_emit, ms_count, ms_compact, ms_glue, ms_total;
    float ms_exchange;            /* multi-GPU: time inside the record and glue exchanges (transport + merge kernels) */
    uint64_t n_launch_scan, n_launch_count, n_launch_compact;   /* workgroups launched */
    uint64_t n_multipass_partitions; /* partitions whose distinct k-mers did not fit one LDS pass (multi-pass kernel) */
    uint64_t n_tiles_overlapped;     /* scan tiles processed while the input was still arriving (cdbg_expect_input) */
    uint64_t n_split_buckets;        /* buckets that no LDS tier of the compaction could take and that were split by sub-minimizer (k_split.h) */
    uint64_t n_glue_rounds;          /* multi-GPU sharded glue: query / reply rounds of the distributed list ranking (0: single GPU, or
                                        the replicated exchange -- emit_replicated, or closed chains across ranks) */
    uint64_t n_walked_unitigs;       /* unitigs written by walks from the chain heads (k_walk.h: one GPU, no chain beyond the step limit, no
                                        closed chain); 0: the list-ranking path of k_glue.h glued this run */
    /* ABI 7 -- deferred record placement: the partition space is cut into count_slices ranges; the scan places the records
     * of the first itself and appends the others to streams, which k_place scatters on a second HIP stream WHILE the count stage counts the
     * slice before.  ms_scan_emit is then the scan kernel alone, ms_count the wall from the scan's end to the count stage's end (it contains
     * the waits for the placement), ms_place the busy span of the placement stream (overlapped with ms_count, not a summand of the step). */
    uint64_t n_deferred_records;     /* records that went through the streams (0: the scan placed every record itself) */
    float ms_place;
    int count_slices;                /* 1: no deferral */
} cdbg_stats_t;

/* ABI version: bumped whenever a struct of this header changes.  From version 5 on cdbg_stats_t only ever GROWS AT ITS END;
 * a binding checks cdbg_abi_version() against the header it was written for and sizeof(cdbg_stats_t) against
 * cdbg_stats_sizeof() when it loads the library (bcalm_amd/api.py does), instead of reading fields at stale offsets. */
#define CDBG_ABI_VERSION 12
int cdbg_abi_version(void);
uint64_t cdbg_stats_sizeof(void);

/* error codes */
#define CDBG_OK 0
#define CDBG_E_PARAM (-1)     /* bad parameter (k out of range, ...) */
#define CDBG_E_NODEVICE (-2)  /* no HIP device / HIP call failed: there is NO CPU fallback */
#define CDBG_E_NOMEM (-3)
#define CDBG_E_STATE (-4)     /* stages called out of order */
#define CDBG_E_INTERNAL (-5)

int  cdbg_create(const cdbg_params* params, cdbg_ctx** out);
void cdbg_destroy(cdbg_ctx* ctx);
/* cdbg_destroy hands the context's device buffers of 1 MB and more (the super-k-mer record region: 75 GB at config 3) to a per-device
 * pool of the process, and the next context of the same shape runs on the very same pages: the read scan is sensitive to the physical
 * placement of its region and counters, and every free + re-allocation made it slower.  At most 55 % of the
 * card's memory is held per device (nothing with CDBG_NO_POOL set in the environment); cdbg_release_cached returns everything to the
 * driver -- call it before another library of the same process (torch, RCCL) needs the HBM. */
int cdbg_release_cached(void);
const char* cdbg_last_error(void);

/* Input.  Host ASCII, caller-owned, borrowed for the call; may be called repeatedly.
 * push_reads: read i is bases[offsets[i] .. offsets[i+1]).  push_text: sequences already
 * separated by any byte outside ACGTacgt ('\n', 'N', ...; such bytes break k-mers, like
 * /root/reference/scripts/unitigEvaluator.cpp:130-131). */
int cdbg_push_reads(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_reads);
int cdbg_push_text(cdbg_ctx* ctx, const char* text, uint64_t nbytes);
/* Zero-copy input for multi-threaded parsers (the `bcalm` CLI: N threads on record-aligned slices of a memory-mapped FASTA /
 * FASTQ, one inflate thread per .gz of a file list; README.md:45-50).  cdbg_stage_acquire hands out one of the context's
 * PINNED staging buffers; the caller writes sequence text into it (sequences separated by any byte outside ACGTacgt) and
 * cdbg_stage_commit appends the first `nbytes` of it to the device text with an asynchronous copy (a '\n' is added when the
 * text does not end with a separator: a commit always ends a sequence -- a sequence longer than a buffer is continued in
 * the next one by repeating its last k-1 bases).  nbytes = 0 hands the buffer back unused.  Both calls are thread-safe
 * and may be mixed with the push calls; commits append in the order in which they arrive (the result does not depend on
 * it).  With cdbg_expect_input the scan of the complete tiles is launched from the commits as from the pushes. */
int cdbg_stage_acquire(cdbg_ctx* ctx, char** buf, uint64_t* capacity);
int cdbg_stage_commit(cdbg_ctx* ctx, char* buf, uint64_t nbytes);
/* Optional, before the first push: the (approximate) number of text bytes that will be pushed, e.g. from the file size.
 * The device text is then allocated once, and the read scan starts on the part of the input that has already landed
 * while the caller is still parsing and pushing the rest (single GPU; README.md:45-50 inputs through the CLI). */
int cdbg_expect_input(cdbg_ctx* ctx, uint64_t text_bytes);
/* Synthetic reads generated directly in HBM (BASELINE.md section 2 generator): reads
 * [first_read, first_read + n_reads) of a set of total_reads reads of read_len bases.
 * cfg 0 .. 255: uniform random genome at 30x coverage, 1 % substitutions (the seed).  cfg | 0x100: the same reads over a
 * HOSTILE genome -- two-letter low-complexity blocks (1 in 20), up to 1000 exact copies of one 5 kbp repeat, 50 homopolymer
 * runs of 600 bases, a third of the reads inside 1/40 of the genome (~20x coverage skew).  cfg < 0: every base 'A' (test
 * hook for the abundance ceiling).  oracle/cdbg_oracle.c:orc_synth_reads writes the same bytes. */
int cdbg_generate_reads(cdbg_ctx* ctx, uint64_t first_read, uint64_t n_reads, uint64_t total_reads,
                        uint64_t read_len, int cfg);
/* copy (part of) the resident read text back to the host (tests, FASTA dumps) */
int cdbg_read_text(cdbg_ctx* ctx, uint64_t first_byte, uint64_t nbytes, char* out);

/* The three hot stages, in order.  cdbg_run = count + compact + glue. */
int cdbg_count(cdbg_ctx* ctx);
int cdbg_compact(cdbg_ctx* ctx);
int cdbg_glue(cdbg_ctx* ctx);
int cdbg_run(cdbg_ctx* ctx);
/* forget the results but keep the resident reads and all device buffers, so the same job can
 * be run again (benchmark steps) without allocator traffic */
int cdbg_reset(cdbg_ctx* ctx);

/* ---- Multi-GPU: one context per GPU (one process per GPU, or one host thread per GPU in one process) ----
 * The reference has nothing here (GraphUnitigsTemplate<span>::create is one shared-memory call, src/bcalm_1.cpp:57);
 * the design is SURVEY.md section 8(e).  Rank r owns the minimizer partitions p with p % world_size == r.  cdbg_run /
 * cdbg_count / cdbg_compact / cdbg_glue of a context with world_size > 1 perform, through the context's transport:
 *   count   reads_replicated = 0 (X1): scan the own SHARD of the reads into super-k-mer records of ALL partitions (one capped
 *           pass, regions squeezed into the owner-major layout), all-to-all-v the records to the partition owners, count the
 *           own partitions.  reads_replicated = 1 (X0): scan ALL reads for the own partitions only; nothing travels.
 *   compact the own buckets (no exchange: the owner of a junction holds every solid k-mer adjacent to it)
 *   glue    emit_replicated = 0: sharded by owner (bcalm_amd/csrc/k_dglue.h) -- every junction record travels once to the rank
 *           its key hashes to, every joined pair once to the owner of the end, list ranking runs on the owners of the pieces
 *           with one query / reply exchange per round, every piece travels once to the owner of its unitig's head; each rank
 *           ends with the unitigs it owns (their union is the graph).  emit_replicated = 1, or closed chains that cross ranks:
 *           the replicated exchange -- pieces + junction log all-gathered, join sharded by key hash with one MAX all-reduce,
 *           chains ranked on every rank; every rank ends with the complete set.
 * A rank that received no reads still takes part in every collective; a rank-local failure is agreed on before the next
 * collective stage, so that every rank returns an error together instead of leaving its peers inside the transport.
 * The transport moves bytes between DEVICE buffers of the ranks.  Built in: RCCL (grouped ncclSend/ncclRecv all-to-all-v,
 * ncclAllGather, ncclAllReduce over xGMI), bound at run time from librccl.so.1:
 *   cdbg_comm_unique_id   rank 0 creates the 128-byte id; the caller distributes it (MPI, torch.distributed, a file)
 *   cdbg_comm_init_rccl   every rank, after cdbg_create on its device
 * or caller-supplied functions (cdbg_set_transport; the CPU tests use gloo and an in-process loop-back).
 * All four functions are collective: every rank calls them in the same order; they return 0 on success.
 *   all_gather_u64  host buffers: n words from every rank, rank order
 *   all_to_all_v    device buffers: send_cnt[r] bytes at send_off[r] go to rank r; recv_cnt[s] bytes from rank s land at recv_off[s]
 *   all_gather_v    device buffers: nbytes of every rank (recv_cnt[s], known from an all_gather_u64) at recv_off[s]   (replicated exchange only)
 *   all_reduce_max_i32  in place on a device buffer of n int32                                                        (replicated exchange only) */
typedef struct cdbg_transport {
    void* user;
    int (*all_gather_u64)(void* user, const uint64_t* send, uint64_t* recv, int n);
    int (*all_to_all_v)(void* user, const void* send_dev, const uint64_t* send_off, const uint64_t* send_cnt,
                        void* recv_dev, const uint64_t* recv_off, const uint64_t* recv_cnt);
    int (*all_gather_v)(void* user, const void* send_dev, uint64_t nbytes, void* recv_dev, const uint64_t* recv_off, const uint64_t* recv_cnt);
    int (*all_reduce_max_i32)(void* user, void* dev, uint64_t n);
} cdbg_transport;
int cdbg_set_transport(cdbg_ctx* ctx, const cdbg_transport* t);
int cdbg_comm_unique_id(void* out_128_bytes);
int cdbg_comm_init_rccl(cdbg_ctx* ctx, const void* unique_id_128_bytes);
/* bytes this rank sent + received through the transport since cdbg_reset (bench.py reports them) */
int cdbg_comm_bytes(cdbg_ctx* ctx, uint64_t* out);

/* Results.  Solid k-mers: kmers has (k+1)-byte stride, NUL-terminated ASCII, canonical strand. */
int cdbg_num_solid(cdbg_ctx* ctx, uint64_t* n);
int cdbg_fetch_solid(cdbg_ctx* ctx, char* kmers, uint32_t* counts, uint64_t capacity, uint64_t* n_written);
/* Unitigs [first, first+n): sequences concatenated into seq_buf (ASCII, no terminators),
 * seq_off[n+1] offsets into seq_buf, kc[n] summed abundances (KC; LN = length,
 * km = KC / (LN-k+1): /root/reference/README.md:62-70).  Orientation and order are
 * unspecified, as in the reference (README.md:84-87). */
int cdbg_num_unitigs(cdbg_ctx* ctx, uint64_t* n, uint64_t* total_bases);
int cdbg_fetch_unitigs(cdbg_ctx* ctx, uint64_t first, uint64_t n, char* seq_buf, uint64_t* seq_off, uint64_t* kc);
/* The same set at 2 bits per base, the form the glue stage leaves resident in HBM next to the ASCII arena (SURVEY.md 8d:
 * "canonical unitigs + KC resident in HBM (2-bit packed)").  All n = cdbg_num_unitigs unitigs at once: `packed` receives
 * ceil(total_bases / 4) bytes of ONE arena; unitig i is bases [base_off[i], base_off[i] + len[i]) of it; base j of the
 * arena = bits [2 (j & 3), 2 (j & 3) + 2) of byte j >> 2, codes A0 C1 G2 T3. */
int cdbg_fetch_unitigs_packed(cdbg_ctx* ctx, uint8_t* packed, uint64_t packed_capacity, uint64_t* base_off, uint32_t* len, uint64_t* kc);
/* per-k-mer abundances of unitigs [first, first+n) (contexts created with all_abundance_counts = 1):
 * ab_off[n+1] offsets into ab; unitig i has LN-k+1 values in the orientation of its sequence
 * (the `ab:Z:` vector of /root/reference/README.md:74-80) */
int cdbg_fetch_unitig_abundances(cdbg_ctx* ctx, uint64_t first, uint64_t n, uint32_t* ab, uint64_t* ab_off);
/* Abundances are 31-bit and saturate: exact below 2^31 - 4096, reported as 2147483647 from there on (KC sums the reported
 * values in 64 bits).  README.md:62-72 (KC = sum of abundances); gatb-core's `-abundance-max` default is the same number. */
int cdbg_stats(cdbg_ctx* ctx, cdbg_stats_t* out);
/* Digests of the resident result, computed on the device (bench.py checks them at sizes no oracle follows):
 * out[0] = sum of KC over the unitigs, out[1] = sum of the solid k-mers' counts (must equal out[0]),
 * out[2] = order- and orientation-independent digest of the set {(unitig, KC)} (formula: k_links.h k_digest_unitigs;
 * pinned against the oracle's unitigs in tests/), out[3] = sum of (LN - k + 1) (must equal n_solid). */
int cdbg_digest(cdbg_ctx* ctx, uint64_t out[4]);
/* The unitig definition (/root/reference/bidirected-graphs-in-bcalm2/bidirected-graphs-in-bcalm2.md:64,83-92) checked on
 * the resident result at any size, by code that shares nothing with the compaction or the glue (bcalm_amd/csrc/k_verify.h):
 *   out[0..2]  k-mer positions of all unitigs, and two independent commutative 64-bit sums over their canonical k-mers
 *   out[3..5]  the same three numbers over the solid k-mers as the count stage left them
 *              -- equal triples <=> the unitigs spell every solid k-mer exactly once and nothing else
 *   out[6]     ends e, f of two different unitigs that are each other's ONLY link (counted from both ends): must be 0 --
 *              every unitig is maximal; builds the links (cdbg_link) when they are not there yet
 *   out[7]     unitigs whose two ends are each other's only link (closed chains, cut open once: legitimate)
 * Several ranks: the sums are additive over the ranks; a rank that holds a share of the unitigs (emit_replicated = 0) has
 * no link table and reports out[6] = out[7] = UINT64_MAX. */
int cdbg_verify(cdbg_ctx* ctx, uint64_t out[8]);
/* Edge conservation: the inner-junction half of the unitig definition (bidirected-graphs-in-bcalm2.md:85 -- "for every
 * 0 < i < n the only edges incident on v_i are e_{i-1}, e_i and their mirrors") at any size.  cdbg_verify's maximality pass
 * sees unitig ENDS only; a unitig that runs THROUGH a branching node passes it.  Here the edges of the solid k-mer graph are
 * counted from the count stage's keys alone (one global table of canonical (k-1)-mers; bcalm_amd/csrc/k_verify.h):
 *   out[0]  D = sum over the ends of all solid k-mers of the k-mer ends they see across their junction
 *   out[1]  L = the same sum over the unitig ENDS (= number of links; builds them when they are not there yet)
 *   out[2]  2 * sum over the unitigs of (LN - k): every inner adjacency of a unitig, seen from both sides
 *   out[3]  distinct junctions of the solid graph
 * out[0] == out[1] + out[2]  <=>  every inner junction of every unitig is 1-in / 1-out (the shortfall of a junction that
 * a unitig runs through wrongly is strictly positive: nothing cancels).  Several ranks: every rank counts a share of the k-mers, their junctions belong to all: UINT64_MAX. */
int cdbg_verify_edges(cdbg_ctx* ctx, uint64_t out[4]);
/* The checks of cdbg_verify (out[0..7]) and cdbg_verify_edges (out[8..11]) for a unitig set SUPPLIED BY THE CALLER -- ASCII
 * bases, offsets[n + 1] -- against the solid k-mers resident after cdbg_count: a FASTA written by any program can be judged
 * against this library's counted k-mer set (and the tests plant an over-compacted unitig to see the edge check fail). */
int cdbg_verify_unitigs(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_unitigs, uint64_t out[12]);

/* Edges between unitigs (the `L:<+/->:<id>:<+/->` tokens of /root/reference/README.md:62-72; GFA `L`
 * lines of scripts/convertToGFA.py:103-112).  After cdbg_glue: cdbg_link builds them on the GPU.
 * cdbg_fetch_links: end_off[2U+1] offsets per unitig END (end 2u = leaving u through the reverse
 * complement of its first k-mer, from-sign '-'; end 2u+1 = leaving through its last k-mer, from-sign
 * '+'); link_to[i] = target end 2v+side: side 0 = enters v at its first k-mer (to-sign '+'),
 * side 1 = enters the reverse complement of its last k-mer (to-sign '-'). */
int cdbg_link(cdbg_ctx* ctx);
int cdbg_num_links(cdbg_ctx* ctx, uint64_t* n);
int cdbg_fetch_links(cdbg_ctx* ctx, uint64_t* end_off, uint32_t* link_to);
/* Several ranks, every rank holding a share of the unitigs (emit_replicated = 0): cdbg_link is COLLECTIVE (all ranks call it).  Unitig
 * ids are then job-wide, numbered rank after rank: this rank's unitig i (the order of cdbg_fetch_unitigs) is first_id + i, end_off
 * covers this rank's ends and link_to holds job-wide end ids (2 x id + side) -- every rank can write its own share of the output
 * file, `L:` tokens included (the bcalm CLI with -nb-gpus does).  One rank, or emit_replicated = 1: first_id = 0, total = this
 * context's unitigs.  After cdbg_link. */
int cdbg_unitig_id_base(cdbg_ctx* ctx, uint64_t* first_id, uint64_t* total);

/* A unitig set SUPPLIED BY THE CALLER becomes the context's resident set, so that its links can be recomputed (the `bcalm -redo-links`
 * mode: pieces cut by split_unitigs / pufferize, whose old links are void; the FASTA of any other program).  Host ASCII: sequence i is
 * bases[offsets[i] .. offsets[i+1]) in ACGTacgt, stored upper-case; every length in [k, 2^32 - 1]; n_unitigs <= 2^31 - 1 (32-bit end ids);
 * kc[n_unitigs] = the KC to keep with each sequence, NULL: all 0.  The bases are checked on the device.  The context must be fresh: no
 * reads pushed or announced, no stage run, world_size == 1 (CDBG_E_STATE otherwise); a bad length or base is CDBG_E_PARAM and the message
 * names the unitig and the byte.
 * Afterwards the context is as after cdbg_glue for cdbg_num_unitigs, cdbg_fetch_unitigs, cdbg_fetch_unitigs_packed, cdbg_link,
 * cdbg_num_links, cdbg_fetch_links, cdbg_unitig_id_base (0 and n) and cdbg_stats (n_unitigs, unitig_bases); cdbg_digest reports out[0],
 * out[2], out[3] and out[1] = UINT64_MAX (no k-mers were counted).  Every call that needs reads, counted k-mers or pieces -- the push,
 * stage and generate calls, cdbg_count / _compact / _glue / _run, cdbg_num_solid, cdbg_fetch_solid, cdbg_fetch_unitig_abundances, the
 * cdbg_verify family -- returns CDBG_E_STATE until cdbg_reset forgets the set.
 * cdbg_link on a loaded context joins WITHOUT a degree bound (bcalm_amd/csrc/k_relink.h): the sequences need not be the unitigs of one
 * graph -- repeated records, self-loops, palindromic (k-1)-mers, any number of ends on one junction.  link_to of every end is in
 * ascending order and the same bytes on every run; the number of links may exceed 2^32; what does not fit in memory is CDBG_E_NOMEM,
 * and so is a set of more than (2^31 - 64) / 3 = 715 827 861 sequences: the load accepts it, cdbg_link cannot address its junction table
 * (at most 2^31 slots, one key per end at two thirds full). */
int cdbg_load_unitigs(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_unitigs, const uint64_t* kc);

/* Node lookup: where is this k-mer -- which unitig, at which offset, on which strand -- or is it not in the graph at all.  Valid after
 * cdbg_glue / cdbg_run and after cdbg_load_unitigs, on one rank (world_size == 1; CDBG_E_STATE otherwise: a rank that holds a share of
 * the unitigs cannot answer for the graph; CDBG_E_STATE too before cdbg_glue).
 * cdbg_index builds the index of the resident unitig set, or keeps the one that is there: an open-address table in HBM of 64-bit slots
 * that hold POSITIONS -- (unitig << 32) | offset, the key of a slot is the k-mer the resident 2-bit arena spells there -- of the smallest
 * power of two >= 1.5 P + 64 slots for the P = sum(LN - k + 1) k-mer positions of the set: 8 bytes per slot for every k
 * (bcalm_amd/csrc/k_index.h).  A table that does not fit is CDBG_E_NOMEM, with the sizes in the message.  cdbg_reset, a new cdbg_glue
 * and a new cdbg_load_unitigs forget the index and hand its memory back.
 * cdbg_index_info (builds the index when it is not there): out[0] = k-mer positions P, out[1] = distinct k-mers, out[2] = slots,
 * out[3] = bytes of the table.  The unitigs of a graph spell every k-mer once: out[0] == out[1] == n_solid; a loaded set may repeat k-mers.
 * cdbg_query (builds the index when it is not there): host ASCII as cdbg_load_unitigs takes it -- sequence i is
 * bases[offsets[i] .. offsets[i+1]), offsets[0] may be non-zero -- and ONE 64-bit word per base: hits[p - offsets[0]] for the k-mer that
 * starts at bases[p]; the caller provides offsets[n_seqs] - offsets[0] words.  n_seqs == 0, or no bases: nothing is written.
 *   hit word           UINT64_MAX = not in the set; otherwise (unitig << 33) | (offset << 1) | strand: unitig = the position in the order of
 *                      cdbg_fetch_unitigs, offset = the first base of the k-mer inside that unitig, strand 0 = the unitig reads there as
 *                      the query k-mer, 1 = as its reverse complement; a k-mer that is its own reverse complement (even k) reports 0.
 *                      With all_abundance_counts the abundance of a hit is ab[ab_off[unitig] + offset] of cdbg_fetch_unitig_abundances.
 *   smallest occurrence  a k-mer that the set spells more than once (loaded sets: repeated records, pieces that overlap, any foreign
 *                      FASTA) reports the smallest (unitig, offset) of its occurrences, and the strand relative to THAT occurrence.
 *   boundaries         bytes outside ACGTacgt break every window that contains them, and every window that does not lie wholly inside one
 *                      sequence is a miss: the last k - 1 positions of each sequence, sequences shorter than k, windows across two
 *                      adjacent sequences whatever the concatenated bytes spell.
 * Device memory per call is bounded: the input is walked in batches of 64 M bases (consecutive batches overlap by k - 1 bases: a sequence
 * may span any number of them) through the pinned staging, and each batch's hits are copied into `hits`. */
int cdbg_index(cdbg_ctx* ctx);
int cdbg_index_info(cdbg_ctx* ctx, uint64_t out[4]);
int cdbg_query(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t* hits);

/* Quantification: how often does a SECOND read set spell the k-mer at every position of every resident unitig, and how much of each
 * unitig does it cover -- the per-sample KC / km / ab:Z: of the header grammar.  Preconditions as for cdbg_query (after cdbg_glue /
 * cdbg_run or cdbg_load_unitigs, one rank; CDBG_E_STATE otherwise).  The library keeps one 32-bit counter per k-mer position of the
 * set (4 bytes x P beside the index; counters that do not fit are CDBG_E_NOMEM, with the sizes in the message), zeroed when created;
 * cdbg_reset, a new cdbg_glue and a new cdbg_load_unitigs forget them with the index.
 * cdbg_quantify (builds the index and the counters when they are not there): input as cdbg_query takes it -- offsets[0] may be non-zero;
 *   empty sequences, sequences shorter than k and bytes outside ACGTacgt are legal.  Every window of k bases that lies wholly inside one
 *   sequence and holds only ACGTacgt adds 1 to the counter of the position cdbg_query reports for it (either strand; in a loaded set
 *   the smallest occurrence); a window that misses adds nothing.  The call ACCUMULATES: two calls equal one call over the concatenated
 *   input.  out (per call, not NULL): out[0] = windows looked at, out[1] = windows found, out[2] = of those, windows answered from the
 *   neighbouring hit without a probe (bcalm_amd/csrc/k_quant.h; 0 in a set that repeats k-mers).  n_seqs == 0, or no bases: the index
 *   and the counters are built, out = {0, 0, 0}.  Device memory per call is bounded as for cdbg_query, with nothing stored per base.
 * cdbg_fetch_quant, unitigs [first, first + n) in the order of cdbg_fetch_unitigs: kc[i] = the sum of the unitig's reported counts,
 *   covered[i] = its positions with a count >= 1 (each may be NULL); ab and ab_off both non-NULL: the per-position counts in the layout
 *   of cdbg_fetch_unitig_abundances -- ab_off[n + 1], LN - k + 1 values per unitig in the orientation of its sequence.  Before any
 *   cdbg_quantify since the set became resident: zeros.
 * cdbg_quant_reset zeroes the counters and keeps the index.
 * Counts follow the abundance rule above: exact below 2^31 - 4096, reported as 2147483647 from there on; kc sums the reported values.
 * (The counters are clamped to that ceiling before 2^31 more windows could be added: none ever wraps.) */
int cdbg_quantify(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t out[3]);
int cdbg_fetch_quant(cdbg_ctx* ctx, uint64_t first, uint64_t n, uint64_t* kc, uint32_t* covered, uint32_t* ab, uint64_t* ab_off);
int cdbg_quant_reset(cdbg_ctx* ctx);

/* Run-length lookup: the WALK of every sequence through the graph -- the maximal runs of consecutive k-mers that lie on one unitig, on one
 * strand, at consecutive offsets -- computed on the device; only the runs come back (bcalm_amd/csrc/k_thread.h).  Preconditions as for
 * cdbg_query (after cdbg_glue / cdbg_run or cdbg_load_unitigs, one rank; CDBG_E_STATE otherwise).
 * A run is defined by the hit words cdbg_query reports, and by nothing else.  Number the positions g of the concatenated text from
 * offsets[0], as hits[] is numbered.  Position g CONTINUES g - 1 when neither hit word is UINT64_MAX, their unitigs are equal, their
 * strands are equal and offset(g) == offset(g - 1) + 1 on strand 0, offset(g - 1) - 1 on strand 1.  A head is a hit that does not continue
 * its predecessor, a tail a hit whose successor does not continue it; the i-th head and the i-th tail, in position order, bound run i:
 *   start   the head's position (relative to offsets[0], as the index into hits[])
 *   place   the head's hit word: (unitig << 33) | (offset << 1) | strand
 *   len     tail - head + 1 windows: unitig `unitig` spells the sequence's bases start .. start + len + k - 2 from `offset` on (strand 0),
 *           or their reverse complement, ending at offset + k (strand 1)
 * Sequence ends and bytes outside ACGTacgt break runs (their windows miss); a k-mer that is its own reverse complement reports strand 0
 * and may therefore cut a strand-1 walk; in a set that repeats k-mers the runs are those of the smallest-occurrence hits.
 * cdbg_thread (builds the index when it is not there): input as cdbg_query takes it.  out (not NULL): out[0] = valid windows, out[1] =
 *   windows found, out[2] = runs, out[3] = windows answered from the neighbouring hit without a probe (0 in a set that repeats k-mers, and
 *   under CDBG_QUANT_NO_EXTEND).  The hit words never leave the device; device memory per call is bounded as for cdbg_query, the result
 *   does not depend on the batch size.  n_seqs == 0, or no bases: success, zeros and no runs.
 * cdbg_fetch_runs: the runs of the LATEST cdbg_thread, which the library keeps in host memory until the next cdbg_thread, cdbg_reset,
 *   cdbg_load_unitigs, cdbg_glue or cdbg_destroy (CDBG_E_STATE when there are none).  run_off[n_seqs + 1]: run_off[i] .. run_off[i + 1]
 *   are the runs of sequence i, in position order; start, place, len: out[2] values each.  Any of the four may be NULL. */
int cdbg_thread(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t out[4]);
int cdbg_fetch_runs(cdbg_ctx* ctx, uint64_t* run_off, uint64_t* start, uint64_t* place, uint32_t* len);

/* Connected components of the unitig graph: which unitigs hang together, how many pieces there are, how big each one is
 * (bcalm_amd/csrc/k_components.h).  Two unitigs share a component exactly when a path of links joins them; sign and direction of the links
 * are ignored, and a unitig whose only links lead to itself is a component of one.  Read-only: nothing that is resident changes.
 * Preconditions as for cdbg_query (after cdbg_glue / cdbg_run or cdbg_load_unitigs, one rank; CDBG_E_STATE otherwise).
 * cdbg_components (builds the links when they are not there, as cdbg_verify does): out (not NULL): out[0] = components, out[1] = unitigs
 *   in the largest component, out[2] = the id of that component (the smallest id on a tie), out[3] = components of exactly one unitig.  An
 *   empty set gives zeros.  Components are numbered 0 .. out[0] - 1 in the order of their smallest unitig: the labels and totals are the
 *   same bytes on every run.  Device memory: 16 bytes per unitig while the call runs, of which the 4 bytes of the label stay, and 36 bytes
 *   per component; what does not fit is CDBG_E_NOMEM with the sizes in the message.
 * cdbg_fetch_components: the result of the LATEST cdbg_components, which the library keeps on the device until cdbg_reset,
 *   cdbg_load_unitigs, cdbg_glue or cdbg_destroy (CDBG_E_STATE when there is none; a repeated cdbg_link does not invalidate it).
 *   comp[n_unitigs] (or NULL): the component of every unitig, in the order of cdbg_fetch_unitigs.  The per-component arrays (n values
 *   each, any may be NULL) cover the components [first, first + n), a range outside [0, out[0]] is CDBG_E_PARAM: first_unitig = the
 *   smallest unitig of the component (strictly ascending), n_unitigs, bases = the sum of the unitigs' lengths, kmers = the sum of
 *   LN - k + 1, kc = the sum of KC. */
int cdbg_components(cdbg_ctx* ctx, uint64_t out[4]);
int cdbg_fetch_components(cdbg_ctx* ctx, uint32_t* comp, uint64_t first, uint64_t n, uint32_t* first_unitig, uint64_t* n_unitigs, uint64_t* bases,
                          uint64_t* kmers, uint64_t* kc);

/* Colours: which of N samples hold the k-mer at every position of every resident unitig, where along a unitig that answer changes, and
 * how many distinct sample sets there are (bcalm_amd/csrc/k_color.h).  Preconditions as for cdbg_query (after cdbg_glue / cdbg_run or
 * cdbg_load_unitigs, one rank; CDBG_E_STATE otherwise).  Positions are numbered g = kmer_off[u] + offset, as cdbg_fetch_quant lays its
 * counts out.  The library keeps N planes of one bit per position (N x P / 8 bytes beside the index, against 4 x P for one set of
 * cdbg_quantify's counters) and one more for the unitig starts; cdbg_reset, a new cdbg_glue and a new cdbg_load_unitigs forget planes and
 * classes with the index.  The counters of cdbg_quantify and the colours do not touch each other.
 *   COLOUR SET  colour c is in the colour set of position g if some cdbg_color(c, ...) since the last cdbg_color_open held a valid window
 *               (inside one sequence, only ACGTacgt) for which cdbg_query reports g; either strand.  In a set that repeats k-mers only the
 *               smallest occurrence is ever reported: later occurrences keep the empty set.  Marking is idempotent and accumulates.
 *   RUN         a maximal interval [offset, offset + len) of positions of ONE unitig with equal colour sets.  The runs of a unitig partition
 *               its LN - k + 1 positions; positions no sample holds form runs too (the empty set).  Runs are ordered by (unitig, offset).
 *   CLASS       a distinct colour set among the runs, numbered 0, 1, ... in the order of their first run; the empty set is a class like any
 *               other and has a number only if a run has it.
 * All results are the same bytes on every run.
 * cdbg_color_open (builds the index when it is not there): n_colors in 1 .. CDBG_MAX_COLORS (CDBG_E_PARAM otherwise); allocates and zeroes
 *   the planes (CDBG_E_NOMEM with the sizes in the message when they do not fit), forgets earlier colours and any class result.
 * cdbg_color: CDBG_E_STATE before an open, color >= n_colors is CDBG_E_PARAM; input as cdbg_quantify takes it.  out (not NULL) = {windows
 *   looked at, windows found, of those answered from the neighbouring hit without a probe} of this call.  Device memory per call is bounded
 *   as for cdbg_quantify, with nothing stored per base.  Invalidates the class result.
 * cdbg_color_classes (CDBG_E_STATE before an open): out (not NULL) = {runs R, classes C, positions with at least one colour, unitigs that
 *   are one run}; an empty set gives zeros; more than 2^32 - 1 runs is CDBG_E_NOMEM.  A fixed number of launches, whatever the data.
 * cdbg_fetch_color_runs: the result of the LATEST cdbg_color_classes (CDBG_E_STATE without one): run_off[n_unitigs + 1] -- run_off[u] ..
 *   run_off[u + 1] are the runs of unitig u -- and per run its offset, length and class (R values each).  Any array may be NULL.
 * cdbg_fetch_color_classes: classes [first, first + n), a range outside [0, C] is CDBG_E_PARAM: n_colors = colours in the set, runs = runs
 *   that have it, kmers = positions those runs cover (n values each), bits = n x ceil(N / 32) words, colour c of a class in bit c & 31 of
 *   its word c >> 5, padding bits zero.  Any array may be NULL. */
#define CDBG_MAX_COLORS 4096
int cdbg_color_open(cdbg_ctx* ctx, uint32_t n_colors);
int cdbg_color(cdbg_ctx* ctx, uint32_t color, const char* bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t out[3]);
int cdbg_color_classes(cdbg_ctx* ctx, uint64_t out[4]);
int cdbg_fetch_color_runs(cdbg_ctx* ctx, uint64_t* run_off, uint32_t* offset, uint32_t* len, uint32_t* cls);
int cdbg_fetch_color_classes(cdbg_ctx* ctx, uint64_t first, uint64_t n, uint32_t* n_colors, uint64_t* runs, uint64_t* kmers, uint32_t* bits);

/* Colour query (pseudoalignment): which of the N samples a read, a contig or a gene belongs to -- the walk of every sequence through the
 * graph joined with the colour runs, and the fold of the joined pieces per sequence, on the device (bcalm_amd/csrc/k_color_query.h).
 * Input is as cdbg_thread takes it; positions are numbered in the concatenated input from offsets[0]; hit words are as cdbg_query reports.
 *   SEGMENT     position g continues g - 1 when cdbg_thread's definition says so AND both hits lie in the same colour run of the latest
 *               cdbg_color_classes.  A segment is a maximal chain of continuing positions: start = its first position, place = the hit word
 *               of that position, len = its windows, cls = the class of its colour run.  Segments are thread runs cut where the colour set
 *               changes; on strand 1 a segment walks its unitig downwards, so the colour runs of a unitig appear in reverse order.  Segments
 *               lie in position order and none spans two sequences.
 *   PER SEQUENCE i   total_i = max(0, length_i - k + 1): every window counts, a window over a byte outside ACGTacgt is a k-mer the graph
 *               does not have.  found_i = the sum of its segments' len.  count_i[c] = the sum of len over its segments whose class holds c.
 *   REPORTED    colour c is reported for sequence i under (num, den, of_found) when count_i[c] >= 1 and count_i[c] * den >= num * base_i in
 *               64-bit arithmetic, base_i = found_i when of_found != 0 and total_i otherwise.  num = 0: the union of the colours seen;
 *               num = den with of_found: the intersection over the k-mers found.  A sequence with base_i = 0 reports nothing.
 * cdbg_color_query: CDBG_E_STATE before cdbg_color_classes and after anything that forgets the classes (a further cdbg_color,
 *   cdbg_color_open, cdbg_reset, cdbg_run, cdbg_glue, cdbg_load_unitigs: each forgets the query result too).  num > den or den == 0, and a
 *   sequence of more than 2^32 - 1 windows, are CDBG_E_PARAM; what does not fit is CDBG_E_NOMEM with the sizes in the message; a failed
 *   call leaves no result behind.  out (not NULL) = {valid windows, windows found, segments S, sequences with at least one colour reported,
 *   windows answered by extension}.  THE CALL RUNS cdbg_thread ON ITS INPUT and, like another cdbg_thread, replaces that call's result:
 *   cdbg_fetch_runs then reports the runs of these sequences.  A later cdbg_thread does not touch the colour query's own buffers.  Device
 *   memory: 20 bytes per thread run and 16 per sequence while the call runs; 24 bytes per segment and 12 + 4 ceil(N / 32) per sequence stay.
 *   A fixed number of launches, whatever the data; the same bytes on every run.
 * cdbg_fetch_color_query (CDBG_E_STATE without a query): per sequence found, n_colors = colours reported and bits[n_seqs][ceil(N / 32)]
 *   (colour c in bit c & 31 of word c >> 5, padding bits zero); seg_off[n_seqs + 1] -- seg_off[i] .. seg_off[i + 1] are the segments of
 *   sequence i -- and per segment start, place, len, class (S values each).  Any pointer may be NULL.
 * cdbg_fetch_color_query_counts: count_i[c] of the sequences [first, first + n) as counts[n][N]; a range outside [0, n_seqs] is
 *   CDBG_E_PARAM.  The matrix is never kept (n_seqs x N x 4 bytes is 16 GB at a million reads and 4096 colours): the call folds the range
 *   again into a temporary of the range's size. */
int cdbg_color_query(cdbg_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs, uint32_t num, uint32_t den, int of_found, uint64_t out[5]);
int cdbg_fetch_color_query(cdbg_ctx* ctx, uint32_t* found, uint32_t* n_colors, uint32_t* bits, uint64_t* seg_off, uint64_t* seg_start, uint64_t* seg_place,
                           uint32_t* seg_len, uint32_t* seg_class);
int cdbg_fetch_color_query_counts(cdbg_ctx* ctx, uint64_t first, uint64_t n, uint32_t* counts);

/* Environment variables read by the library -- test hooks that force paths an ordinary input does not reach (tests/), not
 * tuning knobs; results are identical with and without them:
 *   CDBG_SCAN_MODE=capped|exact|var  record layout (default: by input size and skew; var = one pass into per-partition regions sized
 *                                 from a quarter-sample, what skewed inputs get)   CDBG_PART_CAP=<n>    capped region size (forces spills)
 *   CDBG_VAR_SCALE=<f>            with var: capacity per sampled record (tiny values force spills)      CDBG_NO_SPLIT=1   overfull buckets through
 *                                 the HBM-table compaction tier instead of the second-level split by sub-minimizer (k_split.h)
 *   CDBG_REPAIR_MAX_PASSES=<n>    LDS pass limit of the spill-repair launch   CDBG_NO_COUNT_TIER2=1     skip the second one-pass count tier
 *   CDBG_GLUE_LOG=1               junction records through the sequential log CDBG_GLUE_TABLE=1         global-table junction join
 *   CDBG_JOIN_LOG_JB=<n>          log2 of the join buckets (0 forces the overflow fallback)
 *   CDBG_FORCE_MULTI=1            run the multi-GPU data path with one rank   CDBG_STAGE_BYTES, CDBG_STREAM_MIN_BYTES, CDBG_STREAM_BATCH_TILES: ingest staging sizes
 *   CDBG_GLUE_REPLICATED=1        the replicated glue exchange for emit_replicated = 0 as well       CDBG_HOST_MARKS=1  wall-clock marks between host-side phases (stderr)
 *   CDBG_POISON_ALLOC=<byte>      every device block newly obtained without a request for zeroing (fresh, or from the process's pool) is
 *                                 filled with that byte (0xFF, 0xA5, ...): no kernel may depend on what a buffer held before.  Read for every
 *                                 new block, never on the path that keeps an existing allocation
 *   CDBG_QUERY_BATCH=<n>          cdbg_query, cdbg_quantify, cdbg_thread, cdbg_color, cdbg_color_query: bases per device batch (floor max(4 k, 256)): a sequence then spans many batches
 *   CDBG_INDEX_LOG2_SLOTS=<n>     cdbg_index: a table of 2^n slots, floored at the smallest power of two > distinct k-mers (and never larger
 *                                 than the default): long probe runs that wrap around the table's end
 *   CDBG_QUANT_CLAMP_WINDOWS=<n>  cdbg_quantify: clamp the counters before more than n windows (default and at most 2^31) were added since the last clamp
 *   CDBG_QUANT_NO_EXTEND=1        cdbg_quantify, cdbg_thread, cdbg_color, cdbg_color_query: every window probes the index (no window answered by extension)
 *   CDBG_QUANT_CEILING=<n>        cdbg_quantify / cdbg_fetch_quant: counts are exact below n (default and at most 2^31 - 4096) and reported as 2147483647
 *                                 from there on.  THE ONE HOOK THAT CHANGES REPORTED VALUES: it brings the saturation rule within reach of a test
 *   CDBG_COLOR_LOG2_SLOTS=<n>     cdbg_color_classes: a class table of 2^n slots, floored at the smallest power of two > runs (and never larger
 *                                 than the default, the smallest power of two >= 2 x runs): long probe chains that wrap around the table's end */

#ifdef __cplusplus
}
#endif
#endif /* CDBG_H */
