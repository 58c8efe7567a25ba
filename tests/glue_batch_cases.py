"""Inputs for the tests of the batched glue records of k_compact_wave (test_hostsim_glue_batch.py, test_gpu_glue_batch.py).

Every case names what its buckets must contain; the simulator test reads that back from the per-bucket trace of the simulator
build (CDBG_SIM_CW_TRACE: table size, bucket, entries, glue records, CONFIRMs among them, pieces, k-mers per piece) and fails when
a case does not reach its condition.  The GPU test runs the same inputs: partitioning and classification are the same code."""
import random

COMP = str.maketrans("ACGT", "TGCA")


def rich_text(k, glen, seed, nerr):
    """a random genome as one read plus `nerr` short reads of it with one substitution each, on either strand (abundance-min 1:
    every error opens a bubble or a tip) -- in the style of _mid_bucket_text, with the record count per bucket set by glen and
    the partitioning"""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(glen))
    reads = [g]
    for _ in range(nerr):
        L = rng.randrange(k + 2, 4 * k); s = rng.randrange(0, glen - L); r = list(g[s:s + L])
        p = rng.randrange(1, L - 1); r[p] = rng.choice([c for c in "ACGT" if c != r[p]])
        r = "".join(r)
        reads.append(r if rng.random() < 0.5 else r[::-1].translate(COMP))
    return "\n".join(reads) + "\n"


def _one_read(k, n, seed):
    return "".join(random.Random(seed).choice("ACGT") for _ in range(n)) + "\n"


# a trace row: (table slots, bucket, entries, records, confirms, pieces, [k-mers of each piece])
def _recs(tsw, pred):
    return lambda rows: any(r[0] == tsw and pred(r[3]) for r in rows)


# name -> (text, k, Graph keywords, {condition name: predicate over the trace rows})
BATCH_CASES = {
    # record counts at the edges of the 64-lane steps, in the first wave tier (512 slots) ...
    "recs_63_64": (rich_text(21, 1000, 3, 0), 21, dict(log2_partitions=3, minimizer_size=16),
                   {"63 records": _recs(512, lambda n: n == 63), "64 records": _recs(512, lambda n: n == 64)}),
    "recs_64_65": (rich_text(21, 1000, 4, 0), 21, dict(log2_partitions=3, minimizer_size=16),
                   {"64 records": _recs(512, lambda n: n == 64), "65 records": _recs(512, lambda n: n == 65)}),
    # ... beyond two steps: the held step plus the remainder loop, error-rich reads, coarse partitioning
    "recs_over_128": (rich_text(19, 2200, 1, 44), 19, dict(log2_partitions=4, minimizer_size=15),
                      {"more than 128 records, 512 slots": _recs(512, lambda n: n > 128)}),
    "recs_over_128_tier2": (rich_text(21, 1000, 0, 20), 21, dict(log2_partitions=2, minimizer_size=16),
                            {"more than 128 records, 1024 slots": _recs(1024, lambda n: n > 128),
                             "257 .. 512 entries in the 1024-slot tier": lambda rows: any(r[0] == 1024 and 257 <= r[2] <= 512 for r in rows)}),
    # one record, and it is a CONFIRM between two travellers: a bucket of CONFIRM records only
    "recs_1_confirm_only": (rich_text(25, 400, 2, 0), 25, dict(log2_partitions=4, minimizer_size=16),
                            {"1 record": _recs(512, lambda n: n == 1),
                             "CONFIRM records only": lambda rows: any(r[3] > 0 and r[4] == r[3] for r in rows)}),
    # no record at all: one error-free read in one bucket
    "recs_0": (_one_read(31, 150, 7), 31, dict(log2_partitions=0),
               {"0 records": lambda rows: len(rows) == 1 and rows[0][3] == 0 and rows[0][5] == 1}),
    # open ends only / open ends and CONFIRMs in one bucket
    "open_only_and_both": (rich_text(31, 1500, 0, 0), 31, dict(log2_partitions=2),
                           {"open ends only": lambda rows: any(r[3] > 0 and r[4] == 0 for r in rows),
                            "open ends and CONFIRMs": lambda rows: any(0 < r[4] < r[3] for r in rows)}),
}

# the input of the two-sink and of the overflow tests: records of both kinds in every tier-0 bucket, one bucket beyond two steps
SINK_CASE = (rich_text(19, 2200, 1, 44), 19, dict(log2_partitions=4, minimizer_size=15))


def _pieces(lengths):
    return lambda rows: set(lengths) <= {n for r in rows for n in r[6]}


def _palindrome_text():
    """even k = 12 with the k-mer ACGTACGTACGT, its own reverse complement, inside random flanks and again at a read's end"""
    rng = random.Random(12)
    f = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    return "\n".join([f(60) + "ACGTACGTACGT" + f(60), f(40) + "ACGTACGTACGT", "ACGTACGTACGT"]) + "\n"


# shapes of the piece code around the record passes: name -> (text or golden input name, k, abundance-min, Graph keywords, environment, conditions)
SHAPE_CASES = {
    # pieces of 1, 2 and k - m + 1 = 6 k-mers (a whole super-k-mer) in the buckets of one input
    "piece_lengths": (rich_text(21, 1000, 3, 0), 21, 1, dict(log2_partitions=3, minimizer_size=16), {}, {"pieces of 1, 2 and k - m + 1 k-mers": _pieces([1, 2, 6])}),
    # an isolated cycle inside a bucket (one partition: the whole cycle is one cyclic piece; k < 9: byte prefix path).  circ_test1 and circ_test3
    # are one cycle at k = 7; circ_test2 at k = 7 is two linear unitigs (its cycle is cut by a branch) and runs the same passes without one
    "cycle_in_bucket_1": ("circ_test1", 7, 1, dict(log2_partitions=0), {}, {"one cyclic piece": lambda rows: len(rows) == 1 and rows[0][5] == 1 and rows[0][3] == 0}),
    "cycle_in_bucket_2": ("circ_test2", 7, 1, dict(log2_partitions=0), {}, {}),
    "cycle_in_bucket_3": ("circ_test3", 7, 1, dict(log2_partitions=0), {}, {"one cyclic piece": lambda rows: len(rows) == 1 and rows[0][5] == 1 and rows[0][3] == 0}),
    "even_k_palindrome": (_palindrome_text(), 12, 1, dict(log2_partitions=2, minimizer_size=5), {}, {"records": lambda rows: any(r[3] > 0 for r in rows)}),
    "k_below_9": (rich_text(8, 600, 5, 10), 8, 1, dict(log2_partitions=2, minimizer_size=4), {}, {"records": lambda rows: any(r[3] > 0 for r in rows)}),
    "k_55": (rich_text(55, 1500, 6, 20), 55, 1, dict(log2_partitions=3), {}, {"records": lambda rows: any(r[3] > 0 for r in rows)}),
    "k_127": (rich_text(127, 1500, 8, 8), 127, 1, dict(log2_partitions=3), {}, {"records": lambda rows: any(r[3] > 0 for r in rows)}),
    "tier_1024": (rich_text(21, 1000, 0, 20), 21, 1, dict(log2_partitions=2, minimizer_size=16), {"CDBG_CW_TIER2": "1"},
                  {"257 .. 512 entries in the 1024-slot tier": lambda rows: any(r[0] == 1024 and 257 <= r[2] <= 512 and r[3] > 64 for r in rows)}),
    "all_abundance_counts": (rich_text(21, 1000, 4, 20), 21, 1, dict(log2_partitions=3, minimizer_size=16, all_abundance_counts=True), {}, {"records": lambda rows: any(r[3] > 64 for r in rows)}),
}
