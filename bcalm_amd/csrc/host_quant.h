// host_quant.h -- libcdbg.so, host side of cdbg_quantify / cdbg_fetch_quant / cdbg_quant_reset (k_quant.h): the per-position counters
// beside the index, the batched walk of a caller's sequences that feeds them, and their read-out.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

// reported values: exact below the ceiling, 2147483647 from there on (include/cdbg.h "Abundances are 31-bit and saturate")
uint32_t quant_ceiling(const cdbg_ctx* c) {
    const uint64_t top = (1ull << 31) - 4096;
    if (const char* e = c->knobs.get("CDBG_QUANT_CEILING")) return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), top);
    return (uint32_t)top;
}

// the index and one zeroed counter per k-mer position of the set
template <int W>
int quant_ensure(cdbg_ctx* c, const char* what) {
    CK(index_impl<W>(c, what));
    if (c->quant_ready) return CDBG_OK;
    const uint64_t P = c->index_info[0];
    if (const int rc = c->quant_cnt.alloc(P, false)) {
        if (rc != CDBG_E_NOMEM) return rc;
        const std::string why = g_err;
        return fail(CDBG_E_NOMEM, "%s: %llu counters (%llu bytes) for %llu k-mer positions, beside a table of %llu bytes, do not fit: %s", what,
                    (unsigned long long)P, (unsigned long long)(P * sizeof(uint32_t)), (unsigned long long)P, (unsigned long long)c->index_info[3], why.c_str());
    }
    if (P) HIPCK(hipMemsetAsync(c->quant_cnt.p, 0, P * sizeof(uint32_t), c->stream));   // (pool blocks come back dirty)
    HIPCK(hipStreamSynchronize(c->stream));
    c->quant_ready = true; c->quant_tally = 0;
    return CDBG_OK;
}

template <int W>
int quantify_impl(cdbg_ctx* c, const char* bases, const uint64_t* off, uint64_t n, uint64_t* out) {
    CK(index_refuse(c, "cdbg_quantify"));
    out[0] = out[1] = out[2] = 0;
    for (uint64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return fail(CDBG_E_PARAM, "cdbg_quantify: offsets not monotone at sequence %llu", (unsigned long long)i);
    CK(quant_ensure<W>(c, "cdbg_quantify"));
    const uint64_t base0 = n ? off[0] : 0, total = n ? off[n] - base0 : 0;
    if (!total) return CDBG_OK;
    const uint64_t k = (uint64_t)c->k, P = c->index_info[0];
    // bases per device batch (text + sequence ends, nothing per base); consecutive batches overlap by k - 1 bases, and the windows that
    // start in a batch's last k - 1 bases belong to the next one: counted there, and only there
    uint64_t B = 64ull << 20;
    if (const char* e = c->knobs.get("CDBG_QUERY_BATCH")) B = strtoull(e, nullptr, 10);
    B = std::min<uint64_t>(std::max<uint64_t>(B, std::max<uint64_t>(4 * k, 256)), 1ull << 31);
    // no counter may wrap: after a clamp every counter is <= ceiling < 2^31, and at most `limit` <= 2^31 windows are added before the next
    uint64_t limit = 1ull << 31;
    if (const char* e = c->knobs.get("CDBG_QUANT_CLAMP_WINDOWS")) limit = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), 1ull << 31);
    const uint32_t ceiling = quant_ceiling(c);
    // extension only in a set that spells every k-mer once: elsewhere the neighbour of a hit need not be the smallest occurrence
    const int extend = (c->index_info[0] == c->index_info[1] && !c->knobs.get("CDBG_QUANT_NO_EXTEND")) ? 1 : 0;
    CK(ingest_init(c));                                      // the pinned staging pair and its copy stream
    hipStream_t s = c->stream;
    CK(c->quant_out.alloc(4, false));
    HIPCK(hipMemsetAsync(c->quant_out.p, 0, 4 * sizeof(uint64_t), s));
    std::vector<uint32_t> bnd;
    const bool marks = HostMarks::enabled();
    float ms_kernels = 0;
    for (uint64_t b0 = 0; b0 < total;) {
        const uint64_t b1 = std::min(total, b0 + B), nb = b1 - b0;
        const uint64_t n_out = b1 == total ? nb : nb - (k - 1);
        CK(c->q_text.alloc(nb, false));
        int pb = 0; bool busy[2] = { false, false };
        for (uint64_t d = 0; d < nb; d += cdbg_ctx::STAGE_BYTES, pb ^= 1) {
            const uint64_t m = std::min<uint64_t>(cdbg_ctx::STAGE_BYTES, nb - d);
            if (busy[pb]) HIPCK(hipEventSynchronize(c->pin_ev[pb]));
            memcpy(c->pin[pb], bases + base0 + b0 + d, m);
            HIPCK(hipMemcpyAsync(c->q_text.p + d, c->pin[pb], m, hipMemcpyHostToDevice, c->copy_stream));
            HIPCK(hipEventRecord(c->pin_ev[pb], c->copy_stream));
            busy[pb] = true;
        }
        // the sequence ends inside the batch, in its own coordinates (a run of empty sequences is one end), closed by the batch's end
        bnd.clear();
        for (const uint64_t* it = std::upper_bound(off, off + n + 1, base0 + b0); it < off + n + 1 && *it < base0 + b1; ++it) {
            const uint32_t v = (uint32_t)(*it - base0 - b0);
            if (bnd.empty() || bnd.back() != v) bnd.push_back(v);
        }
        bnd.push_back((uint32_t)nb);
        CK(c->q_bnd.alloc(bnd.size(), false));
        HIPCK(hipMemcpy(c->q_bnd.p, bnd.data(), bnd.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCK(hipStreamSynchronize(c->copy_stream));
        if (c->quant_tally + n_out > limit) {
            if (P) CDBG_LAUNCH(k_quant_clamp, std::min<uint64_t>((P + 255) / 256, 1u << 16), 256, s, c->quant_cnt.p, P, ceiling);
            c->quant_tally = 0;
        }
        c->quant_tally += n_out;
        QuantParams qp{};
        qp.text = c->q_text.p; qp.n_text = nb; qp.n_out = n_out; qp.bnd = c->q_bnd.p; qp.n_bnd = (uint32_t)bnd.size(); qp.k = c->k; qp.extend = extend;
        qp.packed = c->unitig_packed.p; qp.unitig_off = c->unitig_off.p; qp.unitig_len = c->unitig_len.p; qp.kmer_off = c->kmer_off.p;
        qp.slots = c->index_slots.p; qp.mask = c->index_info[2] - 1; qp.cnt = c->quant_cnt.p; qp.out = c->quant_out.p;
        Timer t; if (marks) CK(t.start(s));
        CDBG_LAUNCH((k_quant<W>), (n_out + QUANT_TILE - 1) / QUANT_TILE, QUANT_THREADS, s, qp);
        if (marks) { float ms = 0; CK(t.stop(&ms)); ms_kernels += ms; }
        HIPCK(hipStreamSynchronize(s));                      // (the next batch overwrites the text)
        HIPCK(hipGetLastError());
        b0 += n_out;
    }
    CK(read_u64(c->quant_out.p, out, 3));
    if (marks)                                               // dev aid (CDBG_HOST_MARKS=1; bench_micro/quant_timing.py reads it)
        fprintf(stderr, "[quant] positions %llu kernel_ms %.3f windows %llu found %llu extended %llu\n", (unsigned long long)total, ms_kernels,
                (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2]);
    return CDBG_OK;
}

int quant_reset_impl(cdbg_ctx* c) {
    CK(index_refuse(c, "cdbg_quant_reset"));
    if (!c->quant_ready) return CDBG_OK;                     // (no counters yet: a fetch reports zeros as it is)
    const uint64_t P = c->index_info[0];
    if (P) HIPCK(hipMemsetAsync(c->quant_cnt.p, 0, P * sizeof(uint32_t), c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->quant_tally = 0;
    return CDBG_OK;
}

int fetch_quant_impl(cdbg_ctx* c, uint64_t first, uint64_t n, uint64_t* kc, uint32_t* covered, uint32_t* ab, uint64_t* ab_off) {
    CK(index_refuse(c, "cdbg_fetch_quant"));
    if (first + n > c->n_unitigs) return fail(CDBG_E_PARAM, "cdbg_fetch_quant: unitig range out of bounds");
    const bool want_ab = ab && ab_off;
    if (!n) { if (want_ab) ab_off[0] = 0; return CDBG_OK; }
    hipStream_t s = c->stream;
    if (!c->quant_ready) {                                   // nothing was quantified since the set became resident: zeros
        if (kc) memset(kc, 0, n * sizeof(uint64_t));
        if (covered) memset(covered, 0, n * sizeof(uint32_t));
        if (want_ab) {
            std::vector<uint32_t> len(n);
            HIPCK(hipMemcpy(len.data(), c->unitig_len.p + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t w = 0;
            for (uint64_t i = 0; i < n; ++i) { ab_off[i] = w; w += len[i] - (uint32_t)c->k + 1u; }
            ab_off[n] = w;
            memset(ab, 0, w * sizeof(uint32_t));
        }
        return CDBG_OK;
    }
    const uint32_t ceiling = quant_ceiling(c);
    uint64_t pos0 = 0, pos1 = 0;
    CK(read_u64(c->kmer_off.p + first, &pos0)); CK(read_u64(c->kmer_off.p + first + n, &pos1));
    if (kc || covered) {
        CK(c->quant_kc.alloc(n, false)); CK(c->quant_cov.alloc(n, false));
        HIPCK(hipMemsetAsync(c->quant_kc.p, 0, n * sizeof(uint64_t), s));
        HIPCK(hipMemsetAsync(c->quant_cov.p, 0, n * sizeof(uint32_t), s));
        QuantReduceParams rp{ c->quant_cnt.p, c->kmer_off.p, first, first + n, pos0, pos1, ceiling, c->quant_kc.p, c->quant_cov.p };
        if (pos1 > pos0) {
            const uint64_t lanes = (pos1 - pos0 + QUANT_REDUCE_RUN - 1) / QUANT_REDUCE_RUN;
            CDBG_LAUNCH(k_quant_reduce, std::min<uint64_t>((lanes + 255) / 256, 1u << 16), 256, s, rp);
        }
        HIPCK(hipStreamSynchronize(s));
        HIPCK(hipGetLastError());
        if (kc) HIPCK(hipMemcpy(kc, c->quant_kc.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (covered) HIPCK(hipMemcpy(covered, c->quant_cov.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (want_ab) {
        // the counters of unitigs [first, first + n) are consecutive and lie in the orientation of the sequences: the reported values, piece by piece
        HIPCK(hipMemcpy(ab_off, c->kmer_off.p + first, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i <= n; ++i) ab_off[i] -= pos0;
        const uint64_t PIECE = 64ull << 20;
        for (uint64_t d = pos0; d < pos1; d += PIECE) {
            const uint64_t m = std::min(PIECE, pos1 - d);
            CK(c->quant_rep.alloc(m, false));
            CDBG_LAUNCH(k_quant_report, std::min<uint64_t>((m + 255) / 256, 1u << 16), 256, s, (const uint32_t*)(c->quant_cnt.p + d), c->quant_rep.p, m, ceiling);
            HIPCK(hipStreamSynchronize(s));
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpy(ab + (d - pos0), c->quant_rep.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
    }
    return CDBG_OK;
}

}  // namespace
