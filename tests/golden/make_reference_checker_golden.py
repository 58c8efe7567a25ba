#!/usr/bin/env python3
"""Regenerates tests/golden/reference_checker.json: the verdicts of the reference's own k-mer-set checker
(scripts/unitigEvaluator.cpp, compiled into oracle/_ref/unitigEvaluator by `make -C oracle ref`) on the oracle's
unitigs of every input the reference-checker tests use.

Each entry records the checker's two FINAL RESULTS numbers (k-mers of the input, true positives), that it reported
no erroneous, missing or repeated k-mer, and the set digest (tests/parity.py set_digest, the formula of cdbg_digest)
of the unitig set it accepted.  The tests then judge a unitig set by that digest where the checker binary is absent,
and run the checker itself where it is present.

Needs oracle/_ref/unitigEvaluator (only buildable where the reference sources are):
    python tests/golden/make_reference_checker_golden.py
"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
from parity import config2_genome, set_digest  # noqa: E402

EVAL = os.path.join(ROOT, "oracle", "_ref", "unitigEvaluator")

# tests/test_oracle.py test_reference_checker_accepts_oracle_unitigs
ORACLE_CASES = ["tiny_read/21/1", "minitip/21/1", "pufferize_refs/9/1", "circ_test2/7/1", "rand_c/21/1"]
# tests/test_gpu_benchpath.py test_reference_checker_accepts_hip_unitigs / test_reference_checker_on_hostile_reads
CONFIG2_KS = [31, 32, 55, 96, 127]
HOSTILE_CASES = [(31, 150000, 150, 3 | 0x100), (55, 100000, 150, 4 | 0x100), (127, 12000, 1000, 5 | 0x100), (64, 12000, 1000, 5 | 0x100)]


def verdict(unitigs, ref_records, k):
    """the checker on `unitigs` against the k-mers of `ref_records` (one thread: see tests/test_gpu_benchpath.py)"""
    with tempfile.TemporaryDirectory() as t:
        ref = os.path.join(t, "ref.fa"); utg = os.path.join(t, "utg.fa")
        with open(ref, "w") as f:
            f.write("".join(f">r{i}\n{r}\n" for i, r in enumerate(ref_records)))
        with open(utg, "w") as f:
            f.write("".join(f">{i}\n{s}\n" for i, (s, _) in enumerate(unitigs)))
        out = subprocess.run([EVAL, utg, ref, str(k), "1"], capture_output=True, text=True, timeout=3600).stdout
    final = out[out.index("FINAL RESULTS"):]
    nums = re.search(r"FINAL RESULTS:\s*\n(\d+) (\d+)", final)
    err = re.search(r"ERRONEOUS kmers:\s*(\d+)", final); mis = re.search(r"MISSING kmers:\s*(\d+)", final)
    return {"in_ref": int(nums.group(1)), "tp": int(nums.group(2)), "erroneous": int(err.group(1)), "missing": int(mis.group(1)),
            "repeated": "REPEATED" in final, "set_digest": "%016x" % set_digest(unitigs)}


def main():
    if not os.path.exists(EVAL):
        sys.exit("missing %s: run `make -C oracle ref` where the reference sources are" % EVAL)
    orc = oracle_lib.load()
    out = {}
    for key in ORACLE_CASES:
        name, k, amin = key.split("/")
        k = int(k)
        text = oracle_lib.read_input(name)
        got = orc.run(text, k, int(amin))
        reads = [r.upper() for r in re.split(r"[^ACGTacgt]+", text) if len(r) >= k]
        out["oracle/" + key] = dict(verdict(got["unitigs"], reads, k), solid=got["stats"]["solid"])
    genome = config2_genome(orc)
    for k in CONFIG2_KS:
        got = orc.run(genome, k, 1)
        out["config2/%d" % k] = dict(verdict(got["unitigs"], [genome.decode().strip()], k), solid=got["stats"]["solid"])
    for k, n_reads, read_len, cfg in HOSTILE_CASES:
        text = orc.synth_reads(n_reads, read_len, cfg)
        got = orc.run(text, k, 1)
        out["hostile/%d/%d/%d/%d" % (k, n_reads, read_len, cfg)] = dict(verdict(got["unitigs"], [r for r in text.decode().split("\n") if r], k),
                                                                         solid=got["stats"]["solid"])
    with open(os.path.join(HERE, "reference_checker.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
