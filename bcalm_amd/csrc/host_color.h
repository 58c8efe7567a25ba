// host_color.h -- libcdbg.so, host side of cdbg_color_open / cdbg_color / cdbg_color_classes / cdbg_fetch_color_runs /
// cdbg_fetch_color_classes (k_color.h): the bit planes beside the index, the batched walk of a sample's sequences that marks one of them,
// the run and class phases behind one call, and their read-out.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

template <int W>
int color_open_impl(cdbg_ctx* c, uint32_t n_colors) {
    CK(index_refuse(c, "cdbg_color_open"));
    if (n_colors < 1 || n_colors > CDBG_MAX_COLORS) return fail(CDBG_E_PARAM, "cdbg_color_open: %u colours (1 .. %d)", n_colors, CDBG_MAX_COLORS);
    color_forget(c);                                         // (a call that fails leaves no colours behind)
    CK(index_impl<W>(c, "cdbg_color_open"));
    const uint64_t P = c->index_info[0], U = c->n_unitigs, PW = (P + 31) / 32;
    int rc = c->color_planes.alloc((uint64_t)n_colors * PW, false);
    if (rc == CDBG_OK) rc = c->color_ustart.alloc(PW, false);
    if (rc != CDBG_OK) {
        if (rc != CDBG_E_NOMEM) return rc;
        const std::string why = g_err;
        color_forget(c);
        return fail(CDBG_E_NOMEM, "cdbg_color_open: %u planes + 1 of %llu bits (%llu bytes) for %llu k-mer positions, beside a table of %llu bytes, do not fit: %s", n_colors,
                    (unsigned long long)P, (unsigned long long)(((uint64_t)n_colors + 1) * PW * sizeof(uint32_t)), (unsigned long long)P, (unsigned long long)c->index_info[3], why.c_str());
    }
    hipStream_t s = c->stream;
    if (PW) {                                                // (pool blocks come back dirty)
        HIPCK(hipMemsetAsync(c->color_planes.p, 0, (uint64_t)n_colors * PW * sizeof(uint32_t), s));
        HIPCK(hipMemsetAsync(c->color_ustart.p, 0, PW * sizeof(uint32_t), s));
        CDBG_LAUNCH(k_color_ustart, (U + 255) / 256, 256, s, (const uint64_t*)c->kmer_off.p, U, c->color_ustart.p, PW);
    }
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipGetLastError());
    c->color_n = n_colors; c->color_words = PW; c->color_opened = true;
    return CDBG_OK;
}

template <int W>
int color_impl(cdbg_ctx* c, uint32_t color, const char* bases, const uint64_t* off, uint64_t n, uint64_t* out) {
    CK(index_refuse(c, "cdbg_color"));
    out[0] = out[1] = out[2] = 0;
    if (!c->color_opened) return fail(CDBG_E_STATE, "cdbg_color before cdbg_color_open");
    if (color >= c->color_n) return fail(CDBG_E_PARAM, "cdbg_color: colour %u of %u", color, c->color_n);
    CK(check_offsets("cdbg_color", off, n));
    color_classes_forget(c);
    const uint64_t total = n ? off[n] - off[0] : 0;
    if (!total) return CDBG_OK;
    const uint64_t PW = c->color_words;
    hipStream_t s = c->stream;
    CK(c->color_out.alloc(4, false));
    HIPCK(hipMemsetAsync(c->color_out.p, 0, 4 * sizeof(uint64_t), s));
    const bool marks = HostMarks::enabled();
    float ms_kernels = 0;
    // per base of a batch: text + sequence ends, nothing else (marking a window in two batches would be harmless; the totals would count twice)
    CK(window_batches(c, bases, off, n, [&](uint64_t, uint64_t, uint64_t n_out, const WindowParams& wp) -> int {
        ColorMarkParams mp{};
        (WindowParams&)mp = wp; mp.plane = c->color_planes.p + (uint64_t)color * PW; mp.n_words = PW; mp.out = c->color_out.p;
        Timer t; if (marks) CK(t.start(s));
        CDBG_LAUNCH((k_color_mark<W>), (n_out + QUANT_TILE - 1) / QUANT_TILE, QUANT_THREADS, s, mp);
        if (marks) { float ms = 0; CK(t.stop(&ms)); ms_kernels += ms; }
        HIPCK(hipStreamSynchronize(s));                      // (the next batch overwrites the text)
        HIPCK(hipGetLastError());
        return CDBG_OK;
    }));
    uint64_t o[4] = { 0, 0, 0, 0 };
    CK(read_u64(c->color_out.p, o, 4));
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    if (marks)                                               // dev aid (CDBG_HOST_MARKS=1; bench_micro/color_timing.py reads it)
        fprintf(stderr, "[color] positions %llu kernel_ms %.3f windows %llu found %llu extended %llu atomics %llu\n", (unsigned long long)total, ms_kernels,
                (unsigned long long)o[0], (unsigned long long)o[1], (unsigned long long)o[2], (unsigned long long)o[3]);
    return CDBG_OK;
}

int color_classes_impl(cdbg_ctx* c, uint64_t* out) {
    CK(index_refuse(c, "cdbg_color_classes"));
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!c->color_opened) return fail(CDBG_E_STATE, "cdbg_color_classes before cdbg_color_open");
    color_classes_forget(c);                                 // (a call that fails leaves no result behind)
    const uint64_t U = c->n_unitigs, P = c->index_info[0], PW = c->color_words;
    const uint32_t N = c->color_n, NW = (N + 31) / 32;
    // what does not fit is said with its size
    auto room = [&](int rc, const char* what, uint64_t bytes) -> int {
        if (rc != CDBG_E_NOMEM) return rc;
        const std::string why = g_err;
        color_classes_forget(c);
        return fail(CDBG_E_NOMEM, "cdbg_color_classes: %s (%llu bytes; %llu k-mer positions, %u colours) does not fit: %s", what, (unsigned long long)bytes,
                    (unsigned long long)P, N, why.c_str());
    };
    CK(room(c->cl_run_off.alloc(U + 1, true), "run_off[]", (U + 1) * sizeof(uint64_t)));
    if (!U || !P) { c->cl_ready = true; return CDBG_OK; }
    hipStream_t s = c->stream;
    const bool marks = HostMarks::enabled();
    float ms[3] = { 0, 0, 0 };
    Timer t;
    // 1. run heads: the head mask of every word, heads per wave, their scan, the runs' first positions, then offset / len / run_off
    const uint64_t wgrid = (PW + COLOR_THREADS - 1) / COLOR_THREADS, tiles = wgrid * (COLOR_THREADS / 64);
    DBuf<uint32_t> heads, tile_cnt; DBuf<uint64_t> tile_off, start, d;
    CK(room(heads.alloc(PW, false), "heads[]", PW * sizeof(uint32_t)));
    CK(room(tile_cnt.alloc(tiles, false), "tile_cnt[]", tiles * sizeof(uint32_t))); CK(room(tile_off.alloc(tiles + 1, false), "tile_off[]", (tiles + 1) * sizeof(uint64_t)));
    CK(room(d.alloc(2, true), "totals[]", 2 * sizeof(uint64_t)));
    ColorRunParams rp{};
    rp.planes = c->color_planes.p; rp.ustart = c->color_ustart.p; rp.n_words = PW; rp.n_pos = P; rp.n_colors = N;
    rp.heads = heads.p; rp.tile_cnt = tile_cnt.p; rp.tile_off = tile_off.p;
    rp.kmer_off = c->kmer_off.p; rp.unitig_len = c->unitig_len.p; rp.n_unitigs = U; rp.k = c->k; rp.out = d.p;
    if (marks) CK(t.start(s));
    CDBG_LAUNCH(k_color_heads, wgrid, COLOR_THREADS, s, rp);
    CK(exscan_u32(c, tile_cnt.p, tile_off.p, tiles));
    uint64_t R = 0; CK(read_u64(tile_off.p + tiles, &R));
    if (R < U || R > P) { color_classes_forget(c); return fail(CDBG_E_INTERNAL, "cdbg_color_classes: %llu runs of %llu unitigs and %llu k-mer positions", (unsigned long long)R, (unsigned long long)U, (unsigned long long)P); }
    if (R > 0xFFFFFFFFull) { color_classes_forget(c); return fail(CDBG_E_NOMEM, "cdbg_color_classes: %llu runs, more than the 4294967295 a 32-bit run index holds", (unsigned long long)R); }
    CK(room(start.alloc(R, false), "start[]", R * sizeof(uint64_t)));
    CK(room(c->cl_offset.alloc(R, false), "offset[]", R * sizeof(uint32_t))); CK(room(c->cl_len.alloc(R, false), "len[]", R * sizeof(uint32_t)));
    CK(room(c->cl_cls.alloc(R, false), "class[]", R * sizeof(uint32_t)));
    rp.start = start.p; rp.n_runs = R; rp.run_off = c->cl_run_off.p; rp.offset = c->cl_offset.p; rp.len = c->cl_len.p;
    const uint64_t rgrid = (R + COLOR_THREADS - 1) / COLOR_THREADS;
    CDBG_LAUNCH(k_color_emit, wgrid, COLOR_THREADS, s, rp);
    CDBG_LAUNCH(k_color_runs, rgrid, COLOR_THREADS, s, rp);
    if (marks) { CK(t.stop(&ms[0])); CK(t.start(s)); }
    // 2. classes: the table (the smallest power of two >= 2 R; CDBG_COLOR_LOG2_SLOTS, a test hook: 2^n slots, floored at the smallest power
    //    of two > R -- one slot at least stays empty -- and never larger than the default), the representatives, their scan
    uint64_t slots = pow2_at_least(2 * R);
    if (const char* e = c->knobs.get("CDBG_COLOR_LOG2_SLOTS"))
        slots = std::min(slots, std::max<uint64_t>(pow2_at_least(R + 1), 1ull << std::min<uint64_t>(strtoull(e, nullptr, 10), 62)));
    DBuf<uint64_t> table, where, rank; DBuf<uint32_t> rep, c_rep;
    CK(room(table.alloc(slots, false), "the class table", slots * sizeof(uint64_t)));
    CK(room(where.alloc(R, false), "where[]", R * sizeof(uint64_t))); CK(room(rep.alloc(R, false), "rep[]", R * sizeof(uint32_t)));
    CK(room(rank.alloc(R + 1, false), "rank[]", (R + 1) * sizeof(uint64_t)));
    HIPCK(hipMemsetAsync(table.p, 0xFF, slots * sizeof(uint64_t), s));   // (pool blocks come back dirty)
    ColorClassParams cp{};
    cp.planes = c->color_planes.p; cp.n_words = PW; cp.n_colors = N; cp.nw = NW; cp.start = start.p; cp.len = c->cl_len.p; cp.n_runs = R;
    cp.slots = table.p; cp.mask = slots - 1; cp.where = where.p; cp.rep = rep.p; cp.cls = c->cl_cls.p; cp.rank = rank.p;
    CDBG_LAUNCH(k_color_insert, rgrid, COLOR_THREADS, s, cp);
    CDBG_LAUNCH(k_color_rep, rgrid, COLOR_THREADS, s, cp);
    CK(exscan_u32(c, c->cl_cls.p, rank.p, R));
    uint64_t NC = 0; CK(read_u64(rank.p + R, &NC));
    if (marks) { CK(t.stop(&ms[1])); }
    if (!NC || NC > R) { color_classes_forget(c); return fail(CDBG_E_INTERNAL, "cdbg_color_classes: %llu classes of %llu runs", (unsigned long long)NC, (unsigned long long)R); }
    // 3. the class of every run, totals and bit rows per class
    CK(room(c_rep.alloc(NC, false), "first_run[]", NC * sizeof(uint32_t)));
    CK(room(c->cl_runs.alloc(NC, true), "runs[]", NC * sizeof(uint64_t))); CK(room(c->cl_kmers.alloc(NC, true), "kmers[]", NC * sizeof(uint64_t)));
    CK(room(c->cl_ncol.alloc(NC, true), "n_colors[]", NC * sizeof(uint32_t))); CK(room(c->cl_bits.alloc(NC * NW, false), "bits[]", NC * NW * sizeof(uint32_t)));
    cp.n_classes = NC; cp.c_rep = c_rep.p; cp.c_runs = c->cl_runs.p; cp.c_kmers = c->cl_kmers.p; cp.c_ncol = c->cl_ncol.p; cp.c_bits = c->cl_bits.p;
    if (marks) CK(t.start(s));
    CDBG_LAUNCH(k_color_number, rgrid, COLOR_THREADS, s, cp);
    CDBG_LAUNCH(k_color_gather, (NC * NW + 255) / 256, 256, s, cp);
    if (marks) { CK(t.stop(&ms[2])); }
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipGetLastError());
    uint64_t o[2] = { 0, 0 }; CK(read_u64(d.p, o, 2));
    c->color_info[0] = R; c->color_info[1] = NC; c->color_info[2] = o[0]; c->color_info[3] = o[1];
    for (int i = 0; i < 4; ++i) out[i] = c->color_info[i];
    c->cl_ready = true;
    if (marks)                                               // dev aid (CDBG_HOST_MARKS=1; bench_micro/color_timing.py reads it)
        fprintf(stderr, "[color_classes] positions %llu colours %u runs_ms %.3f table_ms %.3f totals_ms %.3f runs %llu classes %llu coloured %llu single %llu slots %llu\n",
                (unsigned long long)P, N, ms[0], ms[1], ms[2], (unsigned long long)R, (unsigned long long)NC, (unsigned long long)o[0], (unsigned long long)o[1], (unsigned long long)slots);
    return CDBG_OK;
}

int fetch_color_runs_impl(cdbg_ctx* c, uint64_t* run_off, uint32_t* offset, uint32_t* len, uint32_t* cls) {
    CK(index_refuse(c, "cdbg_fetch_color_runs"));
    if (!c->cl_ready) return fail(CDBG_E_STATE, "cdbg_fetch_color_runs before cdbg_color_classes");
    const uint64_t R = c->color_info[0];
    if (run_off) HIPCK(hipMemcpy(run_off, c->cl_run_off.p, (c->n_unitigs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (!R) return CDBG_OK;
    if (offset) HIPCK(hipMemcpy(offset, c->cl_offset.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (len) HIPCK(hipMemcpy(len, c->cl_len.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (cls) HIPCK(hipMemcpy(cls, c->cl_cls.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CDBG_OK;
}

int fetch_color_classes_impl(cdbg_ctx* c, uint64_t first, uint64_t n, uint32_t* n_colors, uint64_t* runs, uint64_t* kmers, uint32_t* bits) {
    CK(index_refuse(c, "cdbg_fetch_color_classes"));
    if (!c->cl_ready) return fail(CDBG_E_STATE, "cdbg_fetch_color_classes before cdbg_color_classes");
    const uint64_t NC = c->color_info[1], NW = (c->color_n + 31) / 32;
    if (first > NC || n > NC - first) return fail(CDBG_E_PARAM, "cdbg_fetch_color_classes: classes [%llu, %llu + %llu) of %llu", (unsigned long long)first, (unsigned long long)first, (unsigned long long)n, (unsigned long long)NC);
    if (!n) return CDBG_OK;
    if (n_colors) HIPCK(hipMemcpy(n_colors, c->cl_ncol.p + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (runs) HIPCK(hipMemcpy(runs, c->cl_runs.p + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (kmers) HIPCK(hipMemcpy(kmers, c->cl_kmers.p + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (bits) HIPCK(hipMemcpy(bits, c->cl_bits.p + first * NW, n * NW * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CDBG_OK;
}

}  // namespace
