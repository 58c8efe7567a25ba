// host_window.h -- libcdbg.so, what the host sides of the index consumers share (cdbg_query, cdbg_quantify, cdbg_thread, cdbg_color;
// k_window.h on the device): the check of a caller's offsets, the extension rule, and the loop that cuts the caller's bases into device
// batches.  Included by cdbg_impl.cpp only, before host_index.h.
#pragma once

namespace {

int check_offsets(const char* what, const uint64_t* off, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return fail(CDBG_E_PARAM, "%s: offsets not monotone at sequence %llu", what, (unsigned long long)i);
    return CDBG_OK;
}

// extension only in a set that spells every k-mer once: elsewhere the neighbour of a hit need not be the smallest occurrence
int window_extend(const cdbg_ctx* c) {
    return (c->index_info[0] == c->index_info[1] && !c->knobs.get("CDBG_QUANT_NO_EXTEND")) ? 1 : 0;
}

// The caller's bases, batch by batch, on the device: q_text holds the batch, q_bnd its sequence ends, and batch(b0, nb, n_out, wp) runs
// with the copy stream drained and wp filled but for `out`.  A batch is CDBG_QUERY_BATCH bases (64 Mi; at least max(4 k, 256)); consecutive
// batches overlap by k - 1 bases, and the windows that start in a batch's last k - 1 bases belong to the next one: b0 advances by
// n_out.  The callable allocates its outputs, launches on c->stream and synchronises it before it returns (the next batch overwrites the
// text).  Needs the index; does nothing for an empty text.
template <class Batch>
int window_batches(cdbg_ctx* c, const char* bases, const uint64_t* off, uint64_t n, Batch&& batch) {
    const uint64_t base0 = n ? off[0] : 0, total = n ? off[n] - base0 : 0;
    if (!total) return CDBG_OK;
    const uint64_t k = (uint64_t)c->k;
    uint64_t B = 64ull << 20;
    if (const char* e = c->knobs.get("CDBG_QUERY_BATCH")) B = strtoull(e, nullptr, 10);
    B = std::min<uint64_t>(std::max<uint64_t>(B, std::max<uint64_t>(4 * k, 256)), 1ull << 31);
    CK(ingest_init(c));                                      // the pinned staging pair and its copy stream
    WindowParams wp{};
    wp.k = c->k; wp.extend = window_extend(c);
    wp.packed = c->unitig_packed.p; wp.unitig_off = c->unitig_off.p; wp.unitig_len = c->unitig_len.p; wp.kmer_off = c->kmer_off.p;
    wp.slots = c->index_slots.p; wp.mask = c->index_info[2] - 1;
    std::vector<uint32_t> bnd;
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
        wp.text = c->q_text.p; wp.n_text = nb; wp.n_out = n_out; wp.bnd = c->q_bnd.p; wp.n_bnd = (uint32_t)bnd.size();
        CK(batch(b0, nb, n_out, wp));
        b0 += n_out;
    }
    return CDBG_OK;
}

}  // namespace
