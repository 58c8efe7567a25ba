"""ctypes binding of libcdbg.so (include/cdbg.h) -- the host-side Python mirror.

Plain pointers and sizes only; torch is not involved.  `load()` opens the HIP build
(bcalm_amd/_build/libcdbg.so); there is no CPU fallback: without the library or
without a HIP device every entry point raises.  (tests/ may pass `path=` to bind the
kernel-logic simulator built by tests/hostsim/build.sh; nothing in this package does.)
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "_build", "libcdbg.so")


E_NOMEM, E_INTERNAL = -3, -5                          # include/cdbg.h CDBG_E_NOMEM, CDBG_E_INTERNAL


class CdbgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcdbg error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("k", C.c_int), ("abundance_min", C.c_int), ("minimizer_size", C.c_int),
                ("log2_partitions", C.c_int), ("device_id", C.c_int), ("world_size", C.c_int),
                ("rank", C.c_int), ("all_abundance_counts", C.c_int), ("emit_replicated", C.c_int), ("reads_replicated", C.c_int)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "input_bytes", "n_records", "n_member_kmers", "n_occurrences", "n_distinct", "n_solid",
        "n_solid_travellers", "n_pieces", "n_glue_open_ends", "n_glue_joined", "n_unitigs",
        "unitig_bases", "n_big_partitions", "n_cycles")] + [
        ("minimizer_size", C.c_int), ("log2_partitions", C.c_int), ("kmer_words", C.c_int)] + [
        (n, C.c_float) for n in ("ms_scan_hist", "ms_scan_emit", "ms_count", "ms_compact", "ms_glue", "ms_total", "ms_exchange")] + [
        (n, C.c_uint64) for n in ("n_launch_scan", "n_launch_count", "n_launch_compact", "n_multipass_partitions", "n_tiles_overlapped", "n_split_buckets", "n_glue_rounds", "n_walked_unitigs", "n_deferred_records")] + [
        ("ms_place", C.c_float), ("count_slices", C.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ABI_VERSION = 12                                       # include/cdbg.h CDBG_ABI_VERSION this binding was written for
EXPORTS = ["cdbg_abi_version", "cdbg_stats_sizeof", "cdbg_create", "cdbg_destroy", "cdbg_release_cached", "cdbg_last_error", "cdbg_push_reads", "cdbg_push_text",
           "cdbg_generate_reads", "cdbg_expect_input", "cdbg_stage_acquire", "cdbg_stage_commit", "cdbg_read_text", "cdbg_count", "cdbg_compact", "cdbg_glue", "cdbg_run", "cdbg_reset",
           "cdbg_num_solid", "cdbg_fetch_solid", "cdbg_num_unitigs", "cdbg_fetch_unitigs", "cdbg_stats", "cdbg_digest", "cdbg_verify",
           "cdbg_verify_edges", "cdbg_verify_unitigs",
           "cdbg_fetch_unitigs_packed", "cdbg_fetch_unitig_abundances", "cdbg_link", "cdbg_num_links", "cdbg_fetch_links", "cdbg_unitig_id_base", "cdbg_load_unitigs", "cdbg_index", "cdbg_index_info", "cdbg_query",
           "cdbg_quantify", "cdbg_fetch_quant", "cdbg_quant_reset", "cdbg_thread", "cdbg_fetch_runs", "cdbg_components", "cdbg_fetch_components",
           "cdbg_color_open", "cdbg_color", "cdbg_color_classes", "cdbg_fetch_color_runs", "cdbg_fetch_color_classes",
           "cdbg_color_query", "cdbg_fetch_color_query", "cdbg_fetch_color_query_counts",
           "cdbg_set_transport", "cdbg_comm_unique_id", "cdbg_comm_init_rccl", "cdbg_comm_bytes"]


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 and looks it up by file name, libcdbg.so
    asks for the soname libamdhip64.so.7: whichever of the two is loaded first decides whether the process ends up
    with one runtime (torch first) or two (libcdbg first; the second one to touch the device then finds no GPU).
    Loading torch's copy before libcdbg.so -- without importing torch -- makes every order work."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        for root in (spec.submodule_search_locations or []) if spec else []:
            cand = os.path.join(root, "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
                return
    except Exception:
        pass                                             # no torch, or not a ROCm build: libcdbg uses the system runtime


def load(path: str | None = None) -> C.CDLL:
    path = path or DEFAULT_LIB
    if not os.path.exists(path):
        raise CdbgError(-2, f"{path} not found: build the HIP extension first "
                            f"(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    if os.path.abspath(path) == os.path.abspath(DEFAULT_LIB):
        _share_hip_runtime_with_torch()
    lib = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    lib.cdbg_stats_sizeof.restype = u64
    if lib.cdbg_abi_version() != ABI_VERSION or lib.cdbg_stats_sizeof() != C.sizeof(Stats):
        raise CdbgError(-1, f"{path}: ABI version {lib.cdbg_abi_version()} / cdbg_stats_t of {lib.cdbg_stats_sizeof()} bytes, "
                            f"this binding expects version {ABI_VERSION} / {C.sizeof(Stats)} bytes")
    lib.cdbg_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    lib.cdbg_destroy.argtypes = [vp]
    lib.cdbg_destroy.restype = None
    lib.cdbg_last_error.restype = C.c_char_p
    lib.cdbg_push_reads.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64]
    lib.cdbg_push_text.argtypes = [vp, C.c_char_p, u64]
    lib.cdbg_generate_reads.argtypes = [vp, u64, u64, u64, u64, i32]
    lib.cdbg_expect_input.argtypes = [vp, u64]
    lib.cdbg_stage_acquire.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    lib.cdbg_stage_commit.argtypes = [vp, vp, u64]
    lib.cdbg_read_text.argtypes = [vp, u64, u64, C.c_char_p]
    for f in ("cdbg_count", "cdbg_compact", "cdbg_glue", "cdbg_run", "cdbg_reset"):
        getattr(lib, f).argtypes = [vp]
    lib.cdbg_num_solid.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_fetch_solid.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), u64, C.POINTER(u64)]
    lib.cdbg_num_unitigs.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.cdbg_fetch_unitigs.argtypes = [vp, u64, u64, C.c_char_p, C.POINTER(u64), C.POINTER(u64)]
    lib.cdbg_fetch_unitigs_packed.argtypes = [vp, C.POINTER(C.c_uint8), u64, C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(u64)]
    lib.cdbg_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.cdbg_digest.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_verify.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_verify_edges.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_verify_unitigs.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64, C.POINTER(u64)]
    lib.cdbg_release_cached.argtypes = []
    lib.cdbg_fetch_unitig_abundances.argtypes = [vp, u64, u64, C.POINTER(C.c_uint32), C.POINTER(u64)]
    lib.cdbg_link.argtypes = [vp]
    lib.cdbg_num_links.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_fetch_links.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_uint32)]
    lib.cdbg_unitig_id_base.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.cdbg_load_unitigs.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64, C.POINTER(u64)]
    lib.cdbg_index.argtypes = [vp]
    lib.cdbg_index_info.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_query.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64, C.POINTER(u64)]
    lib.cdbg_quantify.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64, C.POINTER(u64)]
    lib.cdbg_fetch_quant.argtypes = [vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]
    lib.cdbg_quant_reset.argtypes = [vp]
    lib.cdbg_thread.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64, C.POINTER(u64)]
    lib.cdbg_fetch_runs.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint32)]
    lib.cdbg_components.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_fetch_components.argtypes = [vp, C.POINTER(C.c_uint32), u64, u64, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    u32 = C.c_uint32
    lib.cdbg_color_open.argtypes = [vp, u32]
    lib.cdbg_color.argtypes = [vp, u32, C.c_char_p, C.POINTER(u64), u64, C.POINTER(u64)]
    lib.cdbg_color_classes.argtypes = [vp, C.POINTER(u64)]
    lib.cdbg_fetch_color_runs.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    lib.cdbg_fetch_color_classes.argtypes = [vp, u64, u64, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
    lib.cdbg_color_query.argtypes = [vp, C.c_char_p, C.POINTER(u64), u64, u32, u32, i32, C.POINTER(u64)]
    lib.cdbg_fetch_color_query.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), C.POINTER(u32)]
    lib.cdbg_fetch_color_query_counts.argtypes = [vp, u64, u64, C.POINTER(u32)]
    lib.cdbg_set_transport.argtypes = [vp, vp]
    lib.cdbg_comm_unique_id.argtypes = [vp]
    lib.cdbg_comm_init_rccl.argtypes = [vp, C.c_char_p]
    lib.cdbg_comm_bytes.argtypes = [vp, C.POINTER(u64)]
    return lib


class Graph:
    """One construction job.  Mirrors the reference's single entry point
    GraphUnitigsTemplate<span>::create(props, false) (/root/reference/src/bcalm_1.cpp:57)
    with its three properties -kmer-size / -abundance-min / -in, staged as
    count() -> compact() -> glue() (or run())."""

    def __init__(self, k: int, abundance_min: int = 2, minimizer_size: int = 0, log2_partitions: int = -1,
                 device_id: int = 0, world_size: int = 1, rank: int = 0, lib: C.CDLL | None = None,
                 all_abundance_counts: bool = False, emit_replicated: bool = False, reads_replicated: bool = False):
        self.lib = lib or load()
        self.k = k
        p = Params(k, abundance_min, minimizer_size, log2_partitions, device_id, world_size, rank, 1 if all_abundance_counts else 0,
                   1 if emit_replicated else 0, 1 if reads_replicated else 0)
        self._h = C.c_void_p()
        self._color = None                                   # (colours opened, totals of cdbg_color_classes or None): see _color_forget()
        self._color_query = None
        self._ck(self.lib.cdbg_create(C.byref(p), C.byref(self._h)))

    def _ck(self, rc):
        if rc != 0:
            raise CdbgError(rc, (self.lib.cdbg_last_error() or b"").decode())

    def close(self):
        if self._h:
            self.lib.cdbg_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- input ----
    def push_text(self, text):
        b = text if isinstance(text, (bytes, bytearray)) else text.encode()
        self._ck(self.lib.cdbg_push_text(self._h, bytes(b), len(b)))

    def stage_text(self, text):
        """push_text through the zero-copy staging calls (cdbg_stage_acquire / cdbg_stage_commit): `text` is cut at sequence
        boundaries into pieces that fit a staging buffer"""
        b = text if isinstance(text, (bytes, bytearray)) else text.encode()
        pos = 0
        while pos < len(b):
            buf, cap = C.c_void_p(), C.c_uint64()
            self._ck(self.lib.cdbg_stage_acquire(self._h, C.byref(buf), C.byref(cap)))
            end = min(len(b), pos + cap.value - 1)
            if end < len(b):
                cut = b.rfind(b"\n", pos, end)
                if cut <= pos:
                    self.lib.cdbg_stage_commit(self._h, buf, 0)
                    raise ValueError("a sequence longer than a staging buffer: split it with a k-1 overlap")
                end = cut + 1
            C.memmove(buf, bytes(b[pos:end]), end - pos)
            self._ck(self.lib.cdbg_stage_commit(self._h, buf, end - pos))
            pos = end

    def expect_input(self, nbytes):
        self._ck(self.lib.cdbg_expect_input(self._h, nbytes))

    def push_reads(self, reads):
        seqs = [r if isinstance(r, bytes) else r.encode() for r in reads]
        offs = (C.c_uint64 * (len(seqs) + 1))()
        acc = 0
        for i, s in enumerate(seqs):
            offs[i] = acc
            acc += len(s)
        offs[len(seqs)] = acc
        self._ck(self.lib.cdbg_push_reads(self._h, b"".join(seqs), offs, len(seqs)))

    def load_unitigs(self, seqs, kc=None):
        """adopt a unitig set of the caller's (sequences as str / bytes in ACGTacgt, each at least k long; kc: one KC per sequence,
        default all 0) as this fresh graph's resident unitigs (cdbg_load_unitigs): links() then joins them without a degree bound,
        unitigs() / unitigs_packed() / digest() / stats() describe them; reset() forgets them"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = 0
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        kcs = None
        if kc is not None:
            if len(kc) != len(bs):
                raise ValueError("kc: one value per sequence")
            kcs = (C.c_uint64 * max(len(bs), 1))(*[int(x) for x in kc])
        self._color_forget()
        self._ck(self.lib.cdbg_load_unitigs(self._h, b"".join(bytes(b) for b in bs), off, len(bs), kcs))

    # ---- node lookup (cdbg_index / cdbg_query) ----
    MISS = 0xFFFFFFFFFFFFFFFF

    def index(self):
        """build the k-mer index of the resident unitig set (after run() / glue() / load_unitigs()); a no-op when it is there"""
        self._ck(self.lib.cdbg_index(self._h))

    def index_info(self) -> dict:
        """{positions, distinct, slots, bytes} of the index (built when it is not there)"""
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.cdbg_index_info(self._h, out))
        return {"positions": out[0], "distinct": out[1], "slots": out[2], "bytes": out[3]}

    def query_raw(self, seqs, first_offset=0):
        """-> (hits, offsets): one 64-bit hit word per base of the concatenated sequences (include/cdbg.h cdbg_query: MISS, or
        unitig << 33 | offset << 1 | strand) as a ctypes array, and the offsets[n + 1] of the sequences in it -- no Python object per
        k-mer.  first_offset: the sequences start that many bytes into the buffer handed to the library (offsets[0] != 0)"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = first_offset
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        hits = (C.c_uint64 * max(acc - first_offset, 1))()
        self._ck(self.lib.cdbg_query(self._h, b"\n" * first_offset + b"".join(bytes(b) for b in bs), off, len(bs), hits))
        return hits, [o - first_offset for o in off]

    def query(self, seqs):
        """-> per sequence the list of its len - k + 1 k-mers' places (empty when shorter than k): None, or (unitig, offset, strand)
        with unitig = the position in unitigs(), offset = the k-mer's first base there, strand "+" (the unitig reads as the k-mer)
        or "-" (as its reverse complement)"""
        hits, off = self.query_raw(seqs)
        out = []
        for i in range(len(off) - 1):
            row = []
            for p in range(off[i], max(off[i], off[i + 1] - self.k + 1)):
                h = hits[p]
                row.append(None if h == self.MISS else (h >> 33, (h >> 1) & 0xFFFFFFFF, "-" if h & 1 else "+"))
            out.append(row)
        return out

    # ---- quantification of a read set against the resident unitigs (cdbg_quantify / cdbg_fetch_quant / cdbg_quant_reset) ----
    def quantify(self, seqs, first_offset=0) -> dict:
        """count the k-mers of `seqs` (str / bytes; any bytes, any lengths) at the positions of the resident unitigs that spell them; the
        counts ACCUMULATE over calls.  -> {windows, found, extended} of this call: valid k-mer windows, those in the set, and those of them
        answered from the neighbouring hit without a probe"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = first_offset
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        out = (C.c_uint64 * 3)()
        self._ck(self.lib.cdbg_quantify(self._h, b"\n" * first_offset + b"".join(bytes(b) for b in bs), off, len(bs), out))
        return {"windows": out[0], "found": out[1], "extended": out[2]}

    def quant_raw(self, per_kmer=True):
        """-> (kc, covered, ab, ab_off) as ctypes arrays over all unitigs (ab, ab_off None without per_kmer): no Python object per k-mer"""
        self._ck(self.lib.cdbg_fetch_quant(self._h, 0, 0, None, None, None, None))       # (the call's own refusal, under its own name)
        n, tb = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.cdbg_num_unitigs(self._h, C.byref(n), C.byref(tb)))
        n, tb = n.value, tb.value
        kc = (C.c_uint64 * max(n, 1))()
        cov = (C.c_uint32 * max(n, 1))()
        ab = (C.c_uint32 * max(tb, 1))() if per_kmer else None
        off = (C.c_uint64 * (n + 1))() if per_kmer else None
        self._ck(self.lib.cdbg_fetch_quant(self._h, 0, n, kc, cov, ab, off))
        return kc, cov, ab, off

    def quant(self, per_kmer=False):
        """-> per unitig (same order as unitigs()) (kc, covered): the sum of its positions' counts and the positions counted at least
        once; per_kmer: (kc, covered, [count per k-mer position, in the orientation of the sequence])"""
        kc, cov, ab, off = self.quant_raw(per_kmer)
        n = (len(off) - 1) if per_kmer else self._num_unitigs()
        if per_kmer:
            return [(kc[i], cov[i], list(ab[off[i]:off[i + 1]])) for i in range(n)]
        return [(kc[i], cov[i]) for i in range(n)]

    def quant_reset(self):
        """zero the counts; the index stays"""
        self._ck(self.lib.cdbg_quant_reset(self._h))

    # ---- run-length lookup: the walk of sequences through the resident unitigs (cdbg_thread / cdbg_fetch_runs) ----
    def thread_raw(self, seqs, first_offset=0):
        """-> (totals, run_off, start, place, len): {windows, found, runs, extended} of the call and the runs as ctypes arrays -- run_off[n + 1]
        per sequence, and per run its first position in the concatenated sequences, the hit word of that position (unitig << 33 | offset << 1
        | strand) and its length in windows.  No Python object per k-mer or per run.  first_offset as query_raw takes it"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = first_offset
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.cdbg_thread(self._h, b"\n" * first_offset + b"".join(bytes(b) for b in bs), off, len(bs), out))
        runs = out[2]
        run_off = (C.c_uint64 * (len(bs) + 1))()
        start, place, ln = (C.c_uint64 * max(runs, 1))(), (C.c_uint64 * max(runs, 1))(), (C.c_uint32 * max(runs, 1))()
        self._ck(self.lib.cdbg_fetch_runs(self._h, run_off, start, place, ln))
        return {"windows": out[0], "found": out[1], "runs": runs, "extended": out[3]}, run_off, start, place, ln

    def thread(self, seqs):
        """-> per sequence the list of its runs (q, unitig, offset, strand, n): n consecutive k-mers from the sequence's window q on lie on
        `unitig` from `offset` on, upwards on strand "+" (the unitig reads as the sequence), downwards on "-" (as its reverse complement)"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        _, run_off, start, place, ln = self.thread_raw(bs)
        out, at = [], 0
        for i, b in enumerate(bs):
            out.append([(start[r] - at, place[r] >> 33, (place[r] >> 1) & 0xFFFFFFFF, "-" if place[r] & 1 else "+", ln[r]) for r in range(run_off[i], run_off[i + 1])])
            at += len(b)
        return out

    # ---- connected components of the unitig graph (cdbg_components / cdbg_fetch_components) ----
    def components_raw(self, first=0, count=None):
        """-> (totals, comp, first_unitig, n_unitigs, bases, kmers, kc): {components, largest, largest_id, singletons} of the resident set,
        the component of every unitig (same order as unitigs()) and the per-component arrays of components [first, first + count) (default:
        all) as ctypes arrays.  Components are numbered in the order of their smallest unitig.  No Python object per unitig"""
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.cdbg_components(self._h, out))
        U, n = self._num_unitigs(), (out[0] - first if count is None else count)
        comp = (C.c_uint32 * max(U, 1))()
        fu = (C.c_uint32 * max(n, 1))()
        nu, bases, kmers, kc = ((C.c_uint64 * max(n, 1))() for _ in range(4))
        self._ck(self.lib.cdbg_fetch_components(self._h, comp, first, n, fu, nu, bases, kmers, kc))
        return {"components": out[0], "largest": out[1], "largest_id": out[2], "singletons": out[3]}, comp, fu, nu, bases, kmers, kc

    def components(self):
        """-> (labels, components): the component of every unitig (same order as unitigs()), and per component
        {first_unitig, unitigs, bases, kmers, kc}: its smallest unitig, its unitigs, the sum of their lengths, of their k-mers, of their KC"""
        tot, comp, fu, nu, bases, kmers, kc = self.components_raw()
        U = self._num_unitigs()
        return list(comp[:U]), [{"first_unitig": fu[i], "unitigs": nu[i], "bases": bases[i], "kmers": kmers[i], "kc": kc[i]} for i in range(tot["components"])]

    # ---- the resident unitigs coloured by sample (cdbg_color_open / cdbg_color / cdbg_color_classes / the two fetches) ----
    def _color_forget(self):
        """what this object remembers of the library's colours; with every call after which the library has none (reset, run, glue, load)"""
        self._color = None
        self._color_query = None                             # (sequences of the latest color_query_raw, or None)

    def color_open(self, n):
        """n bit planes, one per sample, all empty; earlier colours and classes are forgotten"""
        self._color_forget()
        self._ck(self.lib.cdbg_color_open(self._h, n))
        self._color = (n, None)

    def color(self, color, seqs, first_offset=0) -> dict:
        """mark colour `color` at the positions of the resident unitigs that spell the k-mers of `seqs` (str / bytes; any bytes, any
        lengths); marks ACCUMULATE over calls and are idempotent.  -> {windows, found, extended} of this call, as quantify() reports them"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = first_offset
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        out = (C.c_uint64 * 3)()
        if self._color:
            self._color = (self._color[0], None)             # (the library forgets its classes with every further mark)
        self._color_query = None                             # (... and the query result folded from them)
        self._ck(self.lib.cdbg_color(self._h, color, b"\n" * first_offset + b"".join(bytes(b) for b in bs), off, len(bs), out))
        return {"windows": out[0], "found": out[1], "extended": out[2]}

    def _color_totals(self):
        """cdbg_color_classes, once per marked state: -> (colours, (runs, classes, colored, single_run_unitigs)); the fetches below share it"""
        if not self._color or self._color[1] is None:
            out = (C.c_uint64 * 4)()
            self._ck(self.lib.cdbg_color_classes(self._h, out))      # (refuses where there is nothing to fold, an open included)
            if not self._color:
                raise CdbgError(-4, "colours were not opened through this Graph: color_open() first")
            self._color = (self._color[0], tuple(out))
        return self._color

    def color_runs_raw(self):
        """-> (totals, run_off, offset, len, cls): {runs, classes, colored, single_run_unitigs} and the runs as ctypes arrays -- run_off[U + 1]
        per unitig, and per run its offset in the unitig, its length in k-mer positions and its class.  No Python object per run"""
        _, out = self._color_totals()
        U, R = self._num_unitigs(), out[0]
        run_off = (C.c_uint64 * (U + 1))()
        offset, ln, cls = ((C.c_uint32 * max(R, 1))() for _ in range(3))
        self._ck(self.lib.cdbg_fetch_color_runs(self._h, run_off, offset, ln, cls))
        return {"runs": R, "classes": out[1], "colored": out[2], "single_run_unitigs": out[3]}, run_off, offset, ln, cls

    def color_runs(self):
        """-> per unitig (same order as unitigs()) the list of its runs (offset, len, class): maximal intervals of k-mer positions with
        equal colour sets; they partition the unitig's positions"""
        _, run_off, offset, ln, cls = self.color_runs_raw()
        return [[(offset[r], ln[r], cls[r]) for r in range(run_off[u], run_off[u + 1])] for u in range(len(run_off) - 1)]

    def color_classes_raw(self, first=0, count=None):
        """-> (n, n_colors, runs, kmers, bits, words per class): the n classes [first, first + count) (default: all) as ctypes arrays; colour c
        of class i is bit c & 31 of bits[i * words + (c >> 5)]"""
        n_colors, out = self._color_totals()
        n = out[1] - first if count is None else count
        nw = (n_colors + 31) // 32
        ncol, bits = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n * nw, 1))()
        runs, kmers = (C.c_uint64 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
        self._ck(self.lib.cdbg_fetch_color_classes(self._h, first, n, ncol, runs, kmers, bits))
        return n, ncol, runs, kmers, bits, nw

    def color_classes(self):
        """-> per class, in the order of its first run, {"colors": [colour indices], "runs": runs that have it, "kmers": positions they cover}"""
        n, ncol, runs, kmers, bits, nw = self.color_classes_raw()
        return [{"colors": [32 * j + b for j in range(nw) for b in range(32) if (bits[i * nw + j] >> b) & 1], "runs": runs[i], "kmers": kmers[i]} for i in range(n)]

    # ---- pseudoalignment of sequences to the coloured unitigs (cdbg_color_query / cdbg_fetch_color_query / cdbg_fetch_color_query_counts) ----
    def color_query_raw(self, seqs, share=(0, 1), of_found=False, first_offset=0):
        """which colours the sequences belong to -> (totals, found, n_colors, bits, words per row, seg_off, seg_start, seg_place, seg_len,
        seg_class): {windows, found, segments, reported, extended} of the call and ctypes arrays -- per sequence the windows found, the
        colours reported and their bit row (colour c in bit c & 31 of bits[i * words + (c >> 5)]); seg_off[n + 1] and per segment (a thread
        run cut where the colour set changes) its first position in the concatenated sequences, the hit word of that position, its length
        in windows and its class.  share = (num, den): colour c is reported when count[c] >= 1 and count[c] * den >= num * base, base = the
        windows found with of_found, all len - k + 1 windows otherwise; (0, 1) is the union, (1, 1) with of_found the intersection over
        the k-mers found.  Replaces the result of thread_raw().  No Python object per k-mer or per segment"""
        n_colors, _ = self._color_totals()                   # (cdbg_color_classes, once per marked state)
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = first_offset
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        out = (C.c_uint64 * 5)()
        self._color_query = None
        self._ck(self.lib.cdbg_color_query(self._h, b"\n" * first_offset + b"".join(bytes(b) for b in bs), off, len(bs), share[0], share[1], 1 if of_found else 0, out))
        self._color_query = len(bs)
        n, S, nw = len(bs), out[2], (n_colors + 31) // 32
        found, ncol, bits = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n * nw, 1))()
        seg_off = (C.c_uint64 * (n + 1))()
        start, place = (C.c_uint64 * max(S, 1))(), (C.c_uint64 * max(S, 1))()
        ln, cls = (C.c_uint32 * max(S, 1))(), (C.c_uint32 * max(S, 1))()
        self._ck(self.lib.cdbg_fetch_color_query(self._h, found, ncol, bits, seg_off, start, place, ln, cls))
        return ({"windows": out[0], "found": out[1], "segments": S, "reported": out[3], "extended": out[4]}, found, ncol, bits, nw, seg_off, start, place, ln, cls)

    def color_query(self, seqs, share=(0, 1), of_found=False):
        """-> per sequence {"windows": all len - k + 1 of them, "found", "colors": [colour indices reported], "segments": [(q, unitig, offset,
        strand, n, class)]}: n consecutive k-mers from the sequence's window q on lie on `unitig` from `offset` on (upwards on "+", downwards
        on "-") inside one colour run of class `class`"""
        bs = [x if isinstance(x, (bytes, bytearray)) else x.encode() for x in seqs]
        _, found, ncol, bits, nw, seg_off, start, place, ln, cls = self.color_query_raw(bs, share, of_found)
        out, at = [], 0
        for i, b in enumerate(bs):
            out.append({"windows": max(0, len(b) - self.k + 1), "found": found[i],
                        "colors": [32 * j + t for j in range(nw) for t in range(32) if (bits[i * nw + j] >> t) & 1],
                        "segments": [(start[s] - at, place[s] >> 33, (place[s] >> 1) & 0xFFFFFFFF, "-" if place[s] & 1 else "+", ln[s], cls[s])
                                     for s in range(seg_off[i], seg_off[i + 1])]})
            at += len(b)
        return out

    def color_query_counts(self, first=0, count=None):
        """-> (n, counts, colours): count[c] of the sequences [first, first + count) (default: all from first on) of the latest color_query as
        the ctypes array counts[n * colours] -- the windows of sequence first + i whose class holds colour c at counts[i * colours + c]"""
        if self._color_query is None or not self._color:
            self._ck(self.lib.cdbg_fetch_color_query_counts(self._h, 0, 0, None))    # (the call's own refusal, under its own name)
            raise CdbgError(-4, "no colour query was run through this Graph: color_query() first")
        n = self._color_query - first if count is None else count
        N = self._color[0]
        counts = (C.c_uint32 * max(n * N, 1))()
        self._ck(self.lib.cdbg_fetch_color_query_counts(self._h, first, n, counts))
        return n, counts, N

    def _num_unitigs(self):
        n, tb = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.cdbg_num_unitigs(self._h, C.byref(n), C.byref(tb)))
        return n.value

    def generate_reads(self, n_reads, read_len, cfg, first_read=0, total_reads=None):
        total = n_reads if total_reads is None else total_reads
        self._ck(self.lib.cdbg_generate_reads(self._h, first_read, n_reads, total, read_len, cfg))

    def read_text(self, first, n):
        buf = C.create_string_buffer(n)
        self._ck(self.lib.cdbg_read_text(self._h, first, n, buf))
        return buf.raw

    # ---- stages ----
    def count(self):
        self._ck(self.lib.cdbg_count(self._h))

    def compact(self):
        self._ck(self.lib.cdbg_compact(self._h))

    def glue(self):
        self._color_forget()
        self._ck(self.lib.cdbg_glue(self._h))

    def run(self):
        self._color_forget()
        self._ck(self.lib.cdbg_run(self._h))

    def reset(self):
        self._color_forget()
        self._ck(self.lib.cdbg_reset(self._h))

    def unitigs_packed(self):
        """the unitig set at 2 bits per base as the glue stage leaves it in HBM: (arena bytes, base_off[], len[], kc[])"""
        n = C.c_uint64(); tot = C.c_uint64()
        self._ck(self.lib.cdbg_num_unitigs(self._h, C.byref(n), C.byref(tot)))
        nb = (tot.value + 3) // 4
        buf = (C.c_uint8 * max(nb, 1))(); off = (C.c_uint64 * max(n.value, 1))(); ln = (C.c_uint32 * max(n.value, 1))(); kc = (C.c_uint64 * max(n.value, 1))()
        self._ck(self.lib.cdbg_fetch_unitigs_packed(self._h, buf, nb, off, ln, kc))
        return bytes(buf)[:nb], list(off)[:n.value], list(ln)[:n.value], list(kc)[:n.value]

    def unitig_abundances(self):
        """-> per unitig (same order as unitigs()) the list of its k-mers' abundances (ab:Z: vector)"""
        n, tb = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.cdbg_num_unitigs(self._h, C.byref(n), C.byref(tb)))
        n, tb = n.value, tb.value
        if n == 0:
            return []
        ab = (C.c_uint32 * max(tb, 1))()
        off = (C.c_uint64 * (n + 1))()
        self._ck(self.lib.cdbg_fetch_unitig_abundances(self._h, 0, n, ab, off))
        return [list(ab[off[i]:off[i + 1]]) for i in range(n)]

    def unitig_id_base(self):
        """-> (first job-wide unitig id of this rank's share, unitigs of the whole job); after links() / cdbg_link"""
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.cdbg_unitig_id_base(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def links(self):
        """-> per unitig (same order as unitigs()) a list of (from_sign, target_unitig, to_sign); a sharded set (several ranks,
        emit_replicated = 0): collective, and target_unitig is a job-wide id (unitig_id_base() + the position in the owner's unitigs())"""
        self._ck(self.lib.cdbg_link(self._h))
        n, tb = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.cdbg_num_unitigs(self._h, C.byref(n), C.byref(tb)))
        U = n.value
        nl = C.c_uint64()
        self._ck(self.lib.cdbg_num_links(self._h, C.byref(nl)))
        off = (C.c_uint64 * (2 * U + 1))()
        to = (C.c_uint32 * max(nl.value, 1))()
        self._ck(self.lib.cdbg_fetch_links(self._h, off, to))
        out = []
        for u in range(U):
            l = []
            for side, fs in ((1, "+"), (0, "-")):
                for i in range(off[2 * u + side], off[2 * u + side + 1]):
                    t = to[i]
                    l.append((fs, t >> 1, "+" if (t & 1) == 0 else "-"))
            out.append(l)
        return out

    def stats(self) -> dict:
        s = Stats()
        self._ck(self.lib.cdbg_stats(self._h, C.byref(s)))
        return s.as_dict()

    def comm_bytes(self):
        """bytes this rank sent + received through the transport since the last reset()"""
        n = C.c_uint64()
        self._ck(self.lib.cdbg_comm_bytes(self._h, C.byref(n)))
        return n.value

    def digest(self):
        """device-side digests of the result: {kc_sum, solid_count_sum, set_digest, kmers_in_unitigs}"""
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.cdbg_digest(self._h, out))
        return {"kc_sum": out[0], "solid_count_sum": out[1], "set_digest": out[2], "kmers_in_unitigs": out[3]}

    def verify(self, edges=True):
        """the unitig definition checked on the device, without the oracle (cdbg_verify, bcalm_amd/csrc/k_verify.h):
        k-mer multiset of the unitigs == solid set (counts + two commutative sums), and no pair of unitig ends that are each
        other's only link (maximality).  mergeable_ends is None on a rank that holds a share of the unitigs.
        edges: also run the edge-conservation pass (verify_edges: a 12-byte x pow2(3 x n_solid) table).  A graph too large for that
        pass (or a card without room for its table: CDBG_E_NOMEM) reports edges = None -- with the reason under "edges_error" -- instead
        of failing the k-mer-set / maximality verdict; any other failure of the pass raises.  edges=False skips
        the pass."""
        out = (C.c_uint64 * 8)()
        self._ck(self.lib.cdbg_verify(self._h, out))
        e, why = None, None
        if edges:
            try:
                e = self.verify_edges()
            except CdbgError as ex:
                if ex.code != E_NOMEM:
                    raise
                why = str(ex)
        d = self._verify_dict(out, e)
        if why is not None:
            d["edges_error"] = why
        return d

    @staticmethod
    def _verify_dict(out, edges):
        none = 0xFFFFFFFFFFFFFFFF
        return {"unitig_kmers": (out[0], out[1], out[2]), "solid_kmers": (out[3], out[4], out[5]),
                "mergeable_ends": None if out[6] == none else out[6], "closed_chains": None if out[7] == none else out[7],
                "edges": edges}

    def verify_edges(self):
        """edge conservation (cdbg_verify_edges): {graph: D, links: L, inner: 2 sum(LN - k), junctions}; a unitig set whose every
        inner junction is 1-in / 1-out has graph == links + inner.  None on a multi-rank job."""
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.cdbg_verify_edges(self._h, out))
        if out[0] == 0xFFFFFFFFFFFFFFFF:
            return None
        return {"graph": out[0], "links": out[1], "inner": out[2], "junctions": out[3]}

    def verify_unitigs(self, seqs):
        """the checks of verify() for a unitig set supplied by the caller (sequences as str / bytes) against the resident solid k-mers"""
        bs = [x if isinstance(x, bytes) else x.encode() for x in seqs]
        off = (C.c_uint64 * (len(bs) + 1))()
        acc = 0
        for i, b in enumerate(bs):
            off[i] = acc
            acc += len(b)
        off[len(bs)] = acc
        out = (C.c_uint64 * 12)()
        self._ck(self.lib.cdbg_verify_unitigs(self._h, b"".join(bs), off, len(bs), out))
        return self._verify_dict(out, {"graph": out[8], "links": out[9], "inner": out[10], "junctions": out[11]})

    @staticmethod
    def edges_conserved(v):
        e = v["edges"]
        return e is None or e["graph"] == e["links"] + e["inner"]

    def release_cached(self):
        """hand the process-wide pool of device buffers back to the driver (cdbg_release_cached): call after close() when torch,
        RCCL or another library of the same process needs the HBM"""
        self.lib.cdbg_release_cached()

    def solid_kmers(self):
        n = C.c_uint64()
        self._ck(self.lib.cdbg_num_solid(self._h, C.byref(n)))
        n = n.value
        if n == 0:
            return []
        kb = C.create_string_buffer(n * (self.k + 1))
        cnt = (C.c_uint32 * n)()
        nw = C.c_uint64()
        self._ck(self.lib.cdbg_fetch_solid(self._h, kb, cnt, n, C.byref(nw)))
        raw = kb.raw
        k1 = self.k + 1
        return sorted((raw[i * k1:i * k1 + self.k].decode(), cnt[i]) for i in range(nw.value))

    def unitigs(self, first=0, count=None):
        """-> [(sequence, KC)] of unitigs [first, first + count) (default: all) in the library's arbitrary order/orientation"""
        n, tb = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.cdbg_num_unitigs(self._h, C.byref(n), C.byref(tb)))
        n, tb = n.value, tb.value
        if count is not None or first:
            n = max(0, min(n - first, n if count is None else count))
        if n == 0:
            return []
        seq = C.create_string_buffer(max(tb, 1))
        off = (C.c_uint64 * (n + 1))()
        kc = (C.c_uint64 * n)()
        self._ck(self.lib.cdbg_fetch_unitigs(self._h, first, n, seq, off, kc))
        raw = seq.raw
        return [(raw[off[i]:off[i + 1]].decode(), kc[i]) for i in range(n)]
