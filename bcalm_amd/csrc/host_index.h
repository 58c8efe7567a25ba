// host_index.h -- libcdbg.so, host side of cdbg_index / cdbg_index_info / cdbg_query (k_index.h): the position table over the resident
// unitig set, and the batched lookup of a caller's sequences in it.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

// the runs cdbg_thread keeps for cdbg_fetch_runs (host_thread.h)
void thread_forget(cdbg_ctx* c) {
    c->runs_ready = false;
    std::vector<uint64_t>().swap(c->run_off); std::vector<uint64_t>().swap(c->run_start); std::vector<uint64_t>().swap(c->run_place);
    std::vector<uint32_t>().swap(c->run_len);
}

// the labels and totals cdbg_components keeps for cdbg_fetch_components (host_components.h)
void components_forget(cdbg_ctx* c) {
    c->comp_ready = false;
    c->comp.release(); c->comp_first.release(); c->comp_unitigs.release(); c->comp_bases.release(); c->comp_kmers.release(); c->comp_kc.release();
    for (uint64_t& v : c->comp_info) v = 0;
}

// what cdbg_color_query keeps for its two fetches (host_color_query.h): it was folded from the classes and goes with them
void color_query_forget(cdbg_ctx* c) {
    c->cq_ready = false; c->cq_n = 0; c->cq_segs = 0;
    c->cq_seg_off.release(); c->cq_seg_start.release(); c->cq_seg_place.release(); c->cq_seg_len.release(); c->cq_seg_cls.release();
    c->cq_found.release(); c->cq_ncol.release(); c->cq_bits.release();
}

// the runs and classes cdbg_color_classes keeps for the two colour fetches, and the planes of cdbg_color_open (host_color.h)
void color_classes_forget(cdbg_ctx* c) {
    color_query_forget(c);
    c->cl_ready = false;
    c->cl_run_off.release(); c->cl_runs.release(); c->cl_kmers.release(); c->cl_offset.release(); c->cl_len.release(); c->cl_cls.release();
    c->cl_ncol.release(); c->cl_bits.release();
    for (uint64_t& v : c->color_info) v = 0;
}
void color_forget(cdbg_ctx* c) {
    color_classes_forget(c);
    c->color_opened = false; c->color_n = 0; c->color_words = 0; c->color_planes.release(); c->color_ustart.release();
}

// whatever replaces the resident set forgets its index: the table goes back to the pool
void index_forget(cdbg_ctx* c) {
    c->indexed = false; c->index_slots.release(); c->kmer_off.release();
    c->quant_ready = false; c->quant_tally = 0; c->quant_cnt.release();      // the counters of cdbg_quantify go with the table (host_quant.h)
    thread_forget(c);                                                        // ... and so do the runs of cdbg_thread
    components_forget(c);                                                    // ... and the component labels of cdbg_components
    color_forget(c);                                                         // ... and the colour planes, runs and classes
    for (uint64_t& v : c->index_info) v = 0;
}

int index_refuse(const cdbg_ctx* c, const char* what) {
    if (c->prm.world_size != 1 || c->force_multi || c->knobs.get("CDBG_FORCE_MULTI"))
        return fail(CDBG_E_STATE, "%s: one rank only (world_size == 1): a rank that holds a share of the unitigs cannot answer for the graph", what);
    if (c->stage < 3) return fail(CDBG_E_STATE, "%s before cdbg_glue", what);
    return CDBG_OK;
}

template <int W>
int index_impl(cdbg_ctx* c, const char* what) {
    CK(index_refuse(c, what));
    if (c->indexed) return CDBG_OK;
    hipStream_t s = c->stream;
    const uint64_t U = c->n_unitigs;
    DBuf<uint32_t> kcount; DBuf<uint64_t> out;
    DBuf<uint64_t>& kmer_off = c->kmer_off;                  // kept with the table: the numbering of cdbg_quantify's counters
    CK(kcount.alloc(U, false)); CK(kmer_off.alloc(U + 1, false)); CK(out.alloc(4, false));
    IndexParams ip{};
    ip.n_unitigs = U; ip.k = c->k; ip.unitig_off = c->unitig_off.p; ip.unitig_len = c->unitig_len.p; ip.packed = c->unitig_packed.p;
    ip.kcount = kcount.p; ip.kmer_off = kmer_off.p; ip.out = out.p;
    if (U) CDBG_LAUNCH(k_index_lens, (U + INDEX_THREADS - 1) / INDEX_THREADS, INDEX_THREADS, s, ip);
    CK(exscan_u32(c, kcount.p, kmer_off.p, U));
    uint64_t P = 0; CK(read_u64(kmer_off.p + U, &P));
    ip.n_pos = P;
    // slots: the smallest power of two >= 1.5 P + 64.  CDBG_INDEX_LOG2_SLOTS (test hook): a second build into a smaller table, never
    // below the smallest power of two > distinct k-mers -- the first build counted them -- so that one slot at least stays empty
    uint64_t slots = pow2_at_least(P + P / 2 + 64), o[3] = { 0, 0, 0 };
    for (int pass = 0; pass < 2; ++pass) {
        if (const int rc = c->index_slots.alloc(slots, false)) {
            if (rc != CDBG_E_NOMEM) return rc;
            const std::string why = g_err;
            return fail(CDBG_E_NOMEM, "cdbg_index: a table of %llu slots (%llu bytes) for %llu k-mer positions does not fit: %s",
                        (unsigned long long)slots, (unsigned long long)(slots * sizeof(uint64_t)), (unsigned long long)P, why.c_str());
        }
        HIPCK(hipMemsetAsync(c->index_slots.p, 0xFF, slots * sizeof(uint64_t), s));   // (pool blocks come back dirty: on every build)
        HIPCK(hipMemsetAsync(out.p, 0, 4 * sizeof(uint64_t), s));
        ip.slots = c->index_slots.p; ip.mask = slots - 1;
        if (P) {
            const uint64_t lanes = (P + INDEX_RUN - 1) / INDEX_RUN;
            CDBG_LAUNCH((k_index_insert<W>), std::min<uint64_t>((lanes + INDEX_THREADS - 1) / INDEX_THREADS, MAX_GRID), INDEX_THREADS, s, ip);
        }
        HIPCK(hipStreamSynchronize(s));
        HIPCK(hipGetLastError());
        CK(read_u64(out.p, o, 3));
        if (o[2] || o[0] != P) return fail(CDBG_E_INTERNAL, "cdbg_index: %llu of %llu k-mer positions inserted, %llu found no slot (%llu slots)",
                                           (unsigned long long)o[0], (unsigned long long)P, (unsigned long long)o[2], (unsigned long long)slots);
        const char* e = pass == 0 ? c->knobs.get("CDBG_INDEX_LOG2_SLOTS") : nullptr;
        if (!e) break;
        const uint64_t want = std::max<uint64_t>(pow2_at_least(o[1] + 1), 1ull << std::min<uint64_t>(strtoull(e, nullptr, 10), 62));
        if (want >= slots) break;
        slots = want;
    }
    c->index_info[0] = P; c->index_info[1] = o[1]; c->index_info[2] = slots; c->index_info[3] = slots * sizeof(uint64_t);
    c->indexed = true;
    return CDBG_OK;
}

template <int W>
int query_impl(cdbg_ctx* c, const char* bases, const uint64_t* off, uint64_t n, uint64_t* hits) {
    CK(index_refuse(c, "cdbg_query"));
    if (!n) return CDBG_OK;
    CK(check_offsets("cdbg_query", off, n));
    const uint64_t total = off[n] - off[0];
    if (!total) return CDBG_OK;
    CK(index_impl<W>(c, "cdbg_query"));
    hipStream_t s = c->stream;
    const bool marks = HostMarks::enabled();
    float ms_kernels = 0;
#ifdef CDBG_PROFILE_PHASES
    CK(c->q_prof.alloc(2, true));
#else
    CK(c->q_prof.alloc(2, false));
#endif
    // per base of a batch: text + sequence ends + 8 bytes of hits
    CK(window_batches(c, bases, off, n, [&](uint64_t b0, uint64_t, uint64_t n_out, const WindowParams& wp) -> int {
        CK(c->q_hits.alloc(n_out, false));
        QueryParams qp{};
        (WindowParams&)qp = wp; qp.hits = c->q_hits.p; qp.out = c->q_prof.p;
        Timer t; if (marks) CK(t.start(s));
        CDBG_LAUNCH((k_query<W>), (n_out + QUERY_TILE - 1) / QUERY_TILE, QUERY_THREADS, s, qp);
        if (marks) { float ms = 0; CK(t.stop(&ms)); ms_kernels += ms; }
        HIPCK(hipStreamSynchronize(s));
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpy(hits + b0, c->q_hits.p, n_out * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return CDBG_OK;
    }));
    if (marks) {                                             // dev aid (CDBG_HOST_MARKS=1; bench_micro/query_timing.py reads it)
        uint64_t pr[2] = { 0, 0 };
#ifdef CDBG_PROFILE_PHASES
        CK(read_u64(c->q_prof.p, pr, 2));
#endif
        fprintf(stderr, "[query] positions %llu kernel_ms %.3f looked_up %llu slots_read %llu\n", (unsigned long long)total, ms_kernels, (unsigned long long)pr[0], (unsigned long long)pr[1]);
    }
    return CDBG_OK;
}

}  // namespace
