// host_components.h -- libcdbg.so, host side of cdbg_components / cdbg_fetch_components (k_components.h): the four phases behind one call,
// the labels and per-component totals the context keeps on the device, and their read-out.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

template <int W>
int components_impl(cdbg_ctx* c, uint64_t* out) {
    CK(index_refuse(c, "cdbg_components"));
    out[0] = out[1] = out[2] = out[3] = 0;
    components_forget(c);                                    // (a call that fails leaves no result behind)
    if (!c->linked) { if (c->loaded) CK(relink_impl<W>(c)); else CK(link_impl<W>(c)); }
    const uint64_t U = c->n_unitigs, L = c->n_links;
    for (uint64_t& v : c->comp_info) v = 0;
    if (!U) { c->comp_ready = true; return CDBG_OK; }
    hipStream_t s = c->stream;
    // what does not fit is said with its size: 16 bytes per unitig while the call runs (parent, comp, the scanned ranks), 4 of them kept; 36 per component
    auto room = [&](int rc, const char* what, uint64_t bytes) -> int {
        if (rc != CDBG_E_NOMEM) return rc;
        const std::string why = g_err;
        return fail(CDBG_E_NOMEM, "cdbg_components: %s (%llu bytes; %llu unitigs, %llu links) does not fit: %s", what, (unsigned long long)bytes,
                    (unsigned long long)U, (unsigned long long)L, why.c_str());
    };
    DBuf<uint32_t> parent; DBuf<uint64_t> rank, d;
    CK(room(parent.alloc(U, false), "parent[]", U * sizeof(uint32_t)));
    CK(room(c->comp.alloc(U, false), "comp[]", U * sizeof(uint32_t)));
    CK(room(rank.alloc(U + 1, false), "rank[]", (U + 1) * sizeof(uint64_t)));
    CK(d.alloc(3, true));
    CompParams cp{};
    cp.n_unitigs = U; cp.n_links = L; cp.k = c->k; cp.link_off = c->link_off.p; cp.link_to = c->link_to.p;
    cp.unitig_len = c->unitig_len.p; cp.unitig_kc = c->unitig_kc.p; cp.parent = parent.p; cp.comp = c->comp.p; cp.rank = rank.p; cp.out = d.p;
    const bool marks = HostMarks::enabled();
    float ms[4] = { 0, 0, 0, 0 };
    Timer t;
    const uint64_t ugrid = (U + COMP_THREADS - 1) / COMP_THREADS;
    // 1. hook: one pass over the links, whatever the graph's diameter
    if (marks) CK(t.start(s));
    CDBG_LAUNCH(k_comp_init, ugrid, COMP_THREADS, s, cp);
    if (L) {
        const uint64_t lanes = (L + COMP_RUN - 1) / COMP_RUN;
        CDBG_LAUNCH(k_comp_hook, std::min<uint64_t>((lanes + COMP_THREADS - 1) / COMP_THREADS, MAX_GRID), COMP_THREADS, s, cp);
    }
    if (marks) { CK(t.stop(&ms[0])); CK(t.start(s)); }
    // 2. compress
    CDBG_LAUNCH(k_comp_compress, ugrid, COMP_THREADS, s, cp);
    if (marks) { CK(t.stop(&ms[1])); CK(t.start(s)); }
    // 3. number: components in the order of their smallest unitig
    CDBG_LAUNCH(k_comp_flag, ugrid, COMP_THREADS, s, cp);
    CK(exscan_u32(c, c->comp.p, rank.p, U));
    CDBG_LAUNCH(k_comp_number, ugrid, COMP_THREADS, s, cp);
    uint64_t NC = 0; CK(read_u64(rank.p + U, &NC));
    if (marks) { CK(t.stop(&ms[2])); }
    if (!NC || NC > U) return fail(CDBG_E_INTERNAL, "cdbg_components: %llu components of %llu unitigs", (unsigned long long)NC, (unsigned long long)U);
    // 4. totals per component, and the summary
    CK(room(c->comp_first.alloc(NC, false), "first_unitig[]", NC * sizeof(uint32_t)));
    CK(room(c->comp_unitigs.alloc(NC, true), "n_unitigs[]", NC * sizeof(uint64_t))); CK(room(c->comp_bases.alloc(NC, true), "bases[]", NC * sizeof(uint64_t)));
    CK(room(c->comp_kmers.alloc(NC, true), "kmers[]", NC * sizeof(uint64_t))); CK(room(c->comp_kc.alloc(NC, true), "kc[]", NC * sizeof(uint64_t)));
    cp.n_comp = NC; cp.c_first = c->comp_first.p; cp.c_unitigs = c->comp_unitigs.p; cp.c_bases = c->comp_bases.p; cp.c_kmers = c->comp_kmers.p; cp.c_kc = c->comp_kc.p;
    if (marks) CK(t.start(s));
    CDBG_LAUNCH(k_comp_totals, ugrid, COMP_THREADS, s, cp);
    CDBG_LAUNCH(k_comp_summary, (NC + COMP_THREADS - 1) / COMP_THREADS, COMP_THREADS, s, cp);
    if (marks) { CK(t.stop(&ms[3])); }
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipGetLastError());
    uint64_t o[3] = { 0, 0, 0 }; CK(read_u64(d.p, o, 3));
    if (o[2]) return fail(CDBG_E_INTERNAL, "cdbg_components: %llu links lead to a unitig id beyond the %llu resident ones", (unsigned long long)o[2], (unsigned long long)U);
    const uint64_t largest = 0xFFFFFFFFull - (o[1] & 0xFFFFFFFFull);
    if (largest >= NC) return fail(CDBG_E_INTERNAL, "cdbg_components: largest component %llu of %llu", (unsigned long long)largest, (unsigned long long)NC);
    c->comp_info[0] = NC; c->comp_info[1] = o[1] >> 32; c->comp_info[2] = largest; c->comp_info[3] = o[0];
    CK(read_u64(c->comp_kmers.p + largest, &c->comp_info[4]));
    for (int i = 0; i < 4; ++i) out[i] = c->comp_info[i];
    c->comp_ready = true;
    if (marks)                                               // dev aid (CDBG_HOST_MARKS=1; bench_micro/components_timing.py reads it)
        fprintf(stderr, "[components] unitigs %llu links %llu hook_ms %.3f compress_ms %.3f number_ms %.3f totals_ms %.3f components %llu largest %llu singletons %llu largest_kmers %llu\n",
                (unsigned long long)U, (unsigned long long)L, ms[0], ms[1], ms[2], ms[3], (unsigned long long)NC, (unsigned long long)c->comp_info[1],
                (unsigned long long)c->comp_info[3], (unsigned long long)c->comp_info[4]);
    return CDBG_OK;
}

int fetch_components_impl(cdbg_ctx* c, uint32_t* comp, uint64_t first, uint64_t n, uint32_t* first_unitig, uint64_t* n_unitigs, uint64_t* bases, uint64_t* kmers, uint64_t* kc) {
    CK(index_refuse(c, "cdbg_fetch_components"));
    if (!c->comp_ready) return fail(CDBG_E_STATE, "cdbg_fetch_components before cdbg_components");
    const uint64_t NC = c->comp_info[0];
    if (first > NC || n > NC - first) return fail(CDBG_E_PARAM, "cdbg_fetch_components: components [%llu, %llu + %llu) of %llu", (unsigned long long)first, (unsigned long long)first, (unsigned long long)n, (unsigned long long)NC);
    if (comp && c->n_unitigs) HIPCK(hipMemcpy(comp, c->comp.p, c->n_unitigs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!n) return CDBG_OK;
    if (first_unitig) HIPCK(hipMemcpy(first_unitig, c->comp_first.p + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_unitigs) HIPCK(hipMemcpy(n_unitigs, c->comp_unitigs.p + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (bases) HIPCK(hipMemcpy(bases, c->comp_bases.p + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (kmers) HIPCK(hipMemcpy(kmers, c->comp_kmers.p + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (kc) HIPCK(hipMemcpy(kc, c->comp_kc.p + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return CDBG_OK;
}

}  // namespace
