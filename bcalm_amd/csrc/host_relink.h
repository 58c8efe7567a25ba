// host_relink.h -- libcdbg.so, host side of cdbg_load_unitigs and of cdbg_link on a loaded context (k_relink.h): a unitig set the caller
// supplies becomes the context's resident set, and its links are joined without a degree bound.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

// every call that needs what only count / compact / glue leave behind
int refuse_loaded(const cdbg_ctx* c, const char* what) {
    if (c && c->loaded) return fail(CDBG_E_STATE, "%s: the context holds a loaded unitig set (cdbg_load_unitigs), no reads and no counted k-mers; cdbg_reset it first", what);
    return CDBG_OK;
}

int load_unitigs_impl(cdbg_ctx* c, const char* bases, const uint64_t* off, uint64_t n, const uint64_t* kc) {
    if (c->loaded) return fail(CDBG_E_STATE, "cdbg_load_unitigs: the context holds a loaded unitig set already; cdbg_reset it first");
    if (c->stage != 0 || c->reads_final || c->n_dev || c->pin_fill || c->expect_bytes)
        return fail(CDBG_E_STATE, "cdbg_load_unitigs needs a fresh context (no reads pushed or announced, no stage run)");
    if (c->prm.world_size != 1 || c->force_multi || c->knobs.get("CDBG_FORCE_MULTI")) return fail(CDBG_E_STATE, "cdbg_load_unitigs: one rank only (world_size == 1)");
    if (n > 0x7FFFFFFFull) return fail(CDBG_E_PARAM, "cdbg_load_unitigs: %llu unitigs, at most 2^31 - 1 (32-bit end ids)", (unsigned long long)n);
    std::vector<uint64_t> h_off(n + 1); std::vector<uint32_t> h_len(std::max<uint64_t>(n, 1));
    const uint64_t base0 = n ? off[0] : 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return fail(CDBG_E_PARAM, "unitig %llu: offsets not monotone", (unsigned long long)i);
        const uint64_t len = off[i + 1] - off[i];
        if (len < (uint64_t)c->k || len > 0xFFFFFFFFull) return fail(CDBG_E_PARAM, "unitig %llu: length %llu outside [k = %d, 2^32 - 1]", (unsigned long long)i, (unsigned long long)len, c->k);
        h_off[i] = off[i] - base0; h_len[i] = (uint32_t)len;
    }
    const uint64_t total = n ? off[n] - base0 : 0;
    h_off[n] = total;
    hipStream_t s = c->stream;
    const uint64_t ucap = std::max<uint64_t>(n, 1);
    CK(c->unitig_off.alloc(ucap, false)); CK(c->unitig_len.alloc(ucap, false)); CK(c->unitig_kc.alloc(ucap, false));
    CK(c->unitig_bases.alloc(total + 64, false));               // (+ 64: the check and the 2-bit packing pass touch whole chunks)
    if (n) {
        HIPCK(hipMemcpy(c->unitig_off.p, h_off.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(c->unitig_len.p, h_len.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (kc) HIPCK(hipMemcpy(c->unitig_kc.p, kc, n * sizeof(uint64_t), hipMemcpyHostToDevice));
        else HIPCK(hipMemset(c->unitig_kc.p, 0, n * sizeof(uint64_t)));
        HIPCK(hipMemcpy(c->unitig_bases.p, bases + base0, total, hipMemcpyHostToDevice));
    }
    HIPCK(hipMemset(c->unitig_bases.p + total, 'A', 64));
    DBuf<uint64_t> bad; CK(bad.alloc(1, false));
    HIPCK(hipMemset(bad.p, 0xFF, sizeof(uint64_t)));
    const uint64_t chunks = (total + 15) / 16;
    if (chunks) { LoadCheckParams lp{ c->unitig_bases.p, total, bad.p }; CDBG_LAUNCH(k_relink_check, (chunks + RELINK_THREADS - 1) / RELINK_THREADS, RELINK_THREADS, s, lp); }
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipGetLastError());
    uint64_t first_bad = ~0ull; CK(read_u64(bad.p, &first_bad));
    if (first_bad != ~0ull) {                                    // name the byte and its unitig (the host looks at one chunk only)
        uint64_t b = first_bad * 16;
        while (b + 1 < total && base_valid((uint8_t)bases[base0 + b])) ++b;
        const uint64_t u = (uint64_t)(std::upper_bound(h_off.begin(), h_off.end(), b) - h_off.begin()) - 1;
        return fail(CDBG_E_PARAM, "unitig %llu: byte %llu of the set (base %llu of the unitig, value 0x%02x) is not one of ACGTacgt",
                    (unsigned long long)u, (unsigned long long)b, (unsigned long long)(b - h_off[u]), (unsigned)(uint8_t)bases[base0 + b]);
    }
    c->n_unitigs = n; c->unitig_total = total;
    CK(pack_unitigs(c));
    HIPCK(hipStreamSynchronize(s));
    c->st = cdbg_stats_t{}; c->st.n_unitigs = n; c->st.unitig_bases = total; c->st.kmer_words = c->W;
    c->linked = false; c->n_links = 0;
    c->stage = 3; c->loaded = true;
    return CDBG_OK;
}

// cdbg_link of a loaded context: link_off[2U + 1], link_to[n_links] of the resident set (k_relink.h)
template <int W>
int relink_impl(cdbg_ctx* c) {
    if (!c->loaded || c->stage < 3) return fail(CDBG_E_STATE, "cdbg_link before cdbg_glue");
    hipStream_t s = c->stream;
    const uint64_t U = c->n_unitigs, NE = 2 * U;
    // junction table: at most one key per end; half full, two thirds where that would pass the 2^31 slots which 2 slot + flag leaves a 32-bit word:
    // 3 U + 64 <= 2^31, so at most 715 827 861 unitigs (include/cdbg.h says so)
    uint64_t cap64 = pow2_at_least(2 * NE + 64);
    if (cap64 > (1ull << 31)) cap64 = pow2_at_least(NE + NE / 2 + 64);
    if (cap64 > (1ull << 31)) return fail(CDBG_E_NOMEM, "cdbg_link: %llu unitigs need a junction table of more than 2^31 slots (at most 715827861 unitigs)", (unsigned long long)U);
    const uint64_t NC = 2 * cap64;
    DBuf<uint64_t> keys, run_off; DBuf<uint32_t> cnt, runs, sorted, end_own, end_opp, deg;
    CK(keys.alloc(cap64 * W, false)); CK(cnt.alloc(NC, false)); CK(run_off.alloc(NC + 1, false));
    CK(runs.alloc(NE + 1, false)); CK(sorted.alloc(NE + 1, false)); CK(end_own.alloc(NE + 1, false)); CK(end_opp.alloc(NE + 1, false)); CK(deg.alloc(NE + 1, false));
    CK(c->link_off.alloc(NE + 1, true));
    c->n_links = 0;
    if (NE) {
        HIPCK(hipMemsetAsync(keys.p, 0xFF, cap64 * W * sizeof(uint64_t), s));
        HIPCK(hipMemsetAsync(cnt.p, 0, NC * sizeof(uint32_t), s));
        RelinkParams rp{};
        rp.n_unitigs = U; rp.k = c->k; rp.unitig_off = c->unitig_off.p; rp.unitig_len = c->unitig_len.p; rp.bases = c->unitig_bases.p;
        rp.keys = keys.p; rp.mask = (uint32_t)(cap64 - 1); rp.cnt = cnt.p; rp.run_off = run_off.p; rp.runs = runs.p; rp.sorted = sorted.p;
        rp.end_own = end_own.p; rp.end_opp = end_opp.p; rp.deg = deg.p;
        const uint64_t grid = (NE + RELINK_THREADS - 1) / RELINK_THREADS;
        CDBG_LAUNCH((k_relink_insert<W>), grid, RELINK_THREADS, s, rp);
        CK(exscan_u32(c, cnt.p, run_off.p, NC));
        CDBG_LAUNCH(k_relink_scatter, grid, RELINK_THREADS, s, rp);
        CDBG_LAUNCH(k_relink_order, grid, RELINK_THREADS, s, rp);
        CDBG_LAUNCH(k_relink_count, grid, RELINK_THREADS, s, rp);
        CK(exscan_u32(c, deg.p, c->link_off.p, NE));
        CK(read_u64(c->link_off.p + NE, &c->n_links));
        if (c->n_links > (1ull << 40)) { const uint64_t nl = c->n_links; c->n_links = 0; return fail(CDBG_E_NOMEM, "cdbg_link: %llu links do not fit in memory", (unsigned long long)nl); }
        CK(c->link_to.alloc(c->n_links, false));
        rp.link_off = c->link_off.p; rp.link_to = c->link_to.p;
        CDBG_LAUNCH(k_relink_fill, grid, RELINK_THREADS, s, rp);
        HIPCK(hipStreamSynchronize(s));
        HIPCK(hipGetLastError());
    }
    c->unitig_id_base = 0; c->unitig_id_total = U;
    c->linked = true;
    return CDBG_OK;
}

}  // namespace
