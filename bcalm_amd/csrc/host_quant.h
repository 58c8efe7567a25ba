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
    CK(check_offsets("cdbg_quantify", off, n));
    CK(quant_ensure<W>(c, "cdbg_quantify"));
    const uint64_t total = n ? off[n] - off[0] : 0;
    if (!total) return CDBG_OK;
    const uint64_t P = c->index_info[0];
    // no counter may wrap: after a clamp every counter is <= ceiling < 2^31, and at most `limit` <= 2^31 windows are added before the next
    uint64_t limit = 1ull << 31;
    if (const char* e = c->knobs.get("CDBG_QUANT_CLAMP_WINDOWS")) limit = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), 1ull << 31);
    const uint32_t ceiling = quant_ceiling(c);
    hipStream_t s = c->stream;
    CK(c->quant_out.alloc(4, false));
    HIPCK(hipMemsetAsync(c->quant_out.p, 0, 4 * sizeof(uint64_t), s));
    const bool marks = HostMarks::enabled();
    float ms_kernels = 0;
    // per base of a batch: text + sequence ends, nothing else
    CK(window_batches(c, bases, off, n, [&](uint64_t, uint64_t, uint64_t n_out, const WindowParams& wp) -> int {
        if (c->quant_tally + n_out > limit) {
            if (P) CDBG_LAUNCH(k_quant_clamp, std::min<uint64_t>((P + 255) / 256, 1u << 16), 256, s, c->quant_cnt.p, P, ceiling);
            c->quant_tally = 0;
        }
        c->quant_tally += n_out;
        QuantParams qp{};
        (WindowParams&)qp = wp; qp.cnt = c->quant_cnt.p; qp.out = c->quant_out.p;
        Timer t; if (marks) CK(t.start(s));
        CDBG_LAUNCH((k_quant<W>), (n_out + QUANT_TILE - 1) / QUANT_TILE, QUANT_THREADS, s, qp);
        if (marks) { float ms = 0; CK(t.stop(&ms)); ms_kernels += ms; }
        HIPCK(hipStreamSynchronize(s));                      // (the next batch overwrites the text)
        HIPCK(hipGetLastError());
        return CDBG_OK;
    }));
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
