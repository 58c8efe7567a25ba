// host_color_query.h -- libcdbg.so, host side of cdbg_color_query / cdbg_fetch_color_query / cdbg_fetch_color_query_counts
// (k_color_query.h): the thread runs of the caller's sequences from cdbg_thread's own path (host_thread.h, seam join included), put on the
// device, the span / emit / fold launches behind them, and the read-out.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

// what the three kernels read of the resident colour result and of the kept query result
void color_query_resident(cdbg_ctx* c, ColorQueryParams& P) {
    P.cl_run_off = c->cl_run_off.p; P.cl_offset = c->cl_offset.p; P.cl_len = c->cl_len.p; P.cl_cls = c->cl_cls.p; P.cl_bits = c->cl_bits.p;
    P.n_unitigs = c->n_unitigs; P.n_cl_runs = c->color_info[0]; P.n_classes = c->color_info[1]; P.n_colors = c->color_n; P.nw = (c->color_n + 31) / 32;
    P.seg_off = c->cq_seg_off.p; P.seg_start = c->cq_seg_start.p; P.seg_place = c->cq_seg_place.p; P.seg_len = c->cq_seg_len.p; P.seg_cls = c->cq_seg_cls.p;
    P.n_seqs = c->cq_n; P.n_segs = c->cq_segs;
    P.found = c->cq_found.p; P.n_col = c->cq_ncol.p; P.bits = c->cq_bits.p;
}

template <int W>
int color_query_impl(cdbg_ctx* c, const char* bases, const uint64_t* off, uint64_t n, uint32_t num, uint32_t den, int of_found, uint64_t* out) {
    CK(index_refuse(c, "cdbg_color_query"));
    for (int i = 0; i < 5; ++i) out[i] = 0;
    color_query_forget(c);                                   // (a call that fails leaves no result behind)
    if (!c->cl_ready) return fail(CDBG_E_STATE, "cdbg_color_query before cdbg_color_classes");
    if (den < 1 || num > den) return fail(CDBG_E_PARAM, "cdbg_color_query: share %u / %u (0 <= num <= den, den >= 1)", num, den);
    const uint64_t k = (uint64_t)c->k;
    CK(check_offsets("cdbg_color_query", off, n));
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = off[i + 1] - off[i];
        if (len >= k && len - k + 1 > 0xFFFFFFFFull)
            return fail(CDBG_E_PARAM, "cdbg_color_query: sequence %llu has %llu windows, more than the 4294967295 a 32-bit count holds", (unsigned long long)i, (unsigned long long)(len - k + 1));
    }
    // 1. the thread runs, as cdbg_thread leaves them (and as cdbg_fetch_runs now reports them)
    uint64_t t[4];
    CK(thread_impl<W>(c, bases, off, n, t));
    const uint64_t R = c->run_start.size();
    const uint32_t N = c->color_n, NW = (N + 31) / 32;
    uint64_t S = 0;
    // what does not fit is said with its size
    auto room = [&](int rc, const char* what, uint64_t bytes) -> int {
        if (rc != CDBG_E_NOMEM) return rc;
        const std::string why = g_err;
        color_query_forget(c);
        return fail(CDBG_E_NOMEM, "cdbg_color_query: %s (%llu bytes; %llu sequences, %llu thread runs, %llu segments, %u colours) does not fit: %s", what,
                    (unsigned long long)bytes, (unsigned long long)n, (unsigned long long)R, (unsigned long long)S, N, why.c_str());
    };
    std::vector<uint32_t> total(n ? n : 1, 0u);
    for (uint64_t i = 0; i < n; ++i) { const uint64_t len = off[i + 1] - off[i]; total[i] = len >= k ? (uint32_t)(len - k + 1) : 0u; }
    DBuf<uint64_t> d_start, d_place, d_run_off, seg_scan, d_out; DBuf<uint32_t> d_len, span_first, span_n, d_total;
    CK(room(d_start.alloc(R, false), "run start[]", R * sizeof(uint64_t))); CK(room(d_place.alloc(R, false), "run place[]", R * sizeof(uint64_t)));
    CK(room(d_len.alloc(R, false), "run len[]", R * sizeof(uint32_t))); CK(room(d_run_off.alloc(n + 1, false), "run_off[]", (n + 1) * sizeof(uint64_t)));
    CK(room(span_first.alloc(R, false), "first[]", R * sizeof(uint32_t))); CK(room(span_n.alloc(R, false), "segments[]", R * sizeof(uint32_t)));
    CK(room(seg_scan.alloc(R + 1, false), "seg_scan[]", (R + 1) * sizeof(uint64_t))); CK(room(d_total.alloc(n, false), "windows[]", n * sizeof(uint32_t)));
    CK(room(d_out.alloc(1, true), "totals[]", sizeof(uint64_t)));
    if (R) {
        HIPCK(hipMemcpy(d_start.p, c->run_start.data(), R * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_place.p, c->run_place.data(), R * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_len.p, c->run_len.data(), R * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    HIPCK(hipMemcpy(d_run_off.p, c->run_off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (n) HIPCK(hipMemcpy(d_total.p, total.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipStream_t s = c->stream;
    const bool marks = HostMarks::enabled();
    float ms[3] = { 0, 0, 0 };
    Timer tm;
    ColorQueryParams P{};
    color_query_resident(c, P);
    P.run_start = d_start.p; P.run_place = d_place.p; P.run_len = d_len.p; P.n_runs = R; P.run_off = d_run_off.p; P.n_seqs = n;
    P.span_first = span_first.p; P.span_n = span_n.p; P.seg_scan = seg_scan.p;
    // 2. segments per thread run, their scan
    if (marks) CK(tm.start(s));
    if (R) CDBG_LAUNCH(k_cq_span, (R + CQ_THREADS - 1) / CQ_THREADS, CQ_THREADS, s, P);
    CK(exscan_u32(c, span_n.p, seg_scan.p, R));
    CK(read_u64(seg_scan.p + R, &S));
    if (marks) { CK(tm.stop(&ms[0])); }
    if (S < R) return fail(CDBG_E_INTERNAL, "cdbg_color_query: %llu segments of %llu thread runs", (unsigned long long)S, (unsigned long long)R);
    // 3. the segments at their own indices, seg_off per sequence
    CK(room(c->cq_seg_off.alloc(n + 1, false), "seg_off[]", (n + 1) * sizeof(uint64_t)));
    CK(room(c->cq_seg_start.alloc(S, false), "segment start[]", S * sizeof(uint64_t))); CK(room(c->cq_seg_place.alloc(S, false), "segment place[]", S * sizeof(uint64_t)));
    CK(room(c->cq_seg_len.alloc(S, false), "segment len[]", S * sizeof(uint32_t))); CK(room(c->cq_seg_cls.alloc(S, false), "segment class[]", S * sizeof(uint32_t)));
    CK(room(c->cq_found.alloc(n, false), "found[]", n * sizeof(uint32_t))); CK(room(c->cq_ncol.alloc(n, NW > 1), "n_colors[]", n * sizeof(uint32_t)));
    CK(room(c->cq_bits.alloc(n * NW, false), "bits[]", n * NW * sizeof(uint32_t)));
    c->cq_n = n; c->cq_segs = S;
    color_query_resident(c, P);
    P.n_segs = S; P.total = d_total.p; P.num = num; P.den = den; P.of_found = of_found ? 1 : 0; P.first = 0; P.n_fold = n; P.out = d_out.p;
    if (marks) CK(tm.start(s));
    CDBG_LAUNCH(k_cq_emit, (std::max<uint64_t>(S, n + 1) + CQ_THREADS - 1) / CQ_THREADS, CQ_THREADS, s, P);
    if (marks) { CK(tm.stop(&ms[1])); CK(tm.start(s)); }
    // 4. the fold per (sequence, 32 colours)
    if (n) CDBG_LAUNCH((k_cq_fold<false>), (n * NW + CQ_THREADS - 1) / CQ_THREADS, CQ_THREADS, s, P);
    if (marks) { CK(tm.stop(&ms[2])); }
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipGetLastError());
    uint64_t reported = 0; CK(read_u64(d_out.p, &reported));
    out[0] = t[0]; out[1] = t[1]; out[2] = S; out[3] = reported; out[4] = t[3];
    c->cq_ready = true;
    if (marks)                                               // dev aid (CDBG_HOST_MARKS=1; bench_micro/color_query_timing.py reads it)
        fprintf(stderr, "[color_query] sequences %llu colours %u span_ms %.3f emit_ms %.3f fold_ms %.3f windows %llu found %llu runs %llu segments %llu reported %llu\n",
                (unsigned long long)n, N, ms[0], ms[1], ms[2], (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)R, (unsigned long long)S, (unsigned long long)reported);
    return CDBG_OK;
}

int fetch_color_query_impl(cdbg_ctx* c, uint32_t* found, uint32_t* n_colors, uint32_t* bits, uint64_t* seg_off, uint64_t* seg_start, uint64_t* seg_place,
                           uint32_t* seg_len, uint32_t* seg_class) {
    CK(index_refuse(c, "cdbg_fetch_color_query"));
    if (!c->cq_ready) return fail(CDBG_E_STATE, "cdbg_fetch_color_query before cdbg_color_query");
    const uint64_t n = c->cq_n, S = c->cq_segs, NW = (c->color_n + 31) / 32;
    if (seg_off) HIPCK(hipMemcpy(seg_off, c->cq_seg_off.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n) {
        if (found) HIPCK(hipMemcpy(found, c->cq_found.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (n_colors) HIPCK(hipMemcpy(n_colors, c->cq_ncol.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (bits) HIPCK(hipMemcpy(bits, c->cq_bits.p, n * NW * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (S) {
        if (seg_start) HIPCK(hipMemcpy(seg_start, c->cq_seg_start.p, S * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (seg_place) HIPCK(hipMemcpy(seg_place, c->cq_seg_place.p, S * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (seg_len) HIPCK(hipMemcpy(seg_len, c->cq_seg_len.p, S * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (seg_class) HIPCK(hipMemcpy(seg_class, c->cq_seg_cls.p, S * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return CDBG_OK;
}

// the counts matrix is never kept: the rows of the range are folded again from the kept segments into a temporary of the range's size
int fetch_color_query_counts_impl(cdbg_ctx* c, uint64_t first, uint64_t n, uint32_t* counts) {
    CK(index_refuse(c, "cdbg_fetch_color_query_counts"));
    if (!c->cq_ready) return fail(CDBG_E_STATE, "cdbg_fetch_color_query_counts before cdbg_color_query");
    if (first > c->cq_n || n > c->cq_n - first)
        return fail(CDBG_E_PARAM, "cdbg_fetch_color_query_counts: sequences [%llu, %llu + %llu) of %llu", (unsigned long long)first, (unsigned long long)first, (unsigned long long)n, (unsigned long long)c->cq_n);
    if (!n) return CDBG_OK;
    if (!counts) return fail(CDBG_E_PARAM, "null argument");
    const uint64_t N = c->color_n, NW = (N + 31) / 32;
    DBuf<uint32_t> tmp;
    if (const int rc = tmp.alloc(n * N, false)) {
        if (rc != CDBG_E_NOMEM) return rc;
        const std::string why = g_err;
        return fail(CDBG_E_NOMEM, "cdbg_fetch_color_query_counts: counts[] (%llu bytes; %llu sequences, %llu colours) does not fit: %s", (unsigned long long)(n * N * sizeof(uint32_t)),
                    (unsigned long long)n, (unsigned long long)N, why.c_str());
    }
    ColorQueryParams P{};
    color_query_resident(c, P);
    P.first = first; P.n_fold = n; P.counts = tmp.p;
    CDBG_LAUNCH((k_cq_fold<true>), (n * NW + CQ_THREADS - 1) / CQ_THREADS, CQ_THREADS, c->stream, P);
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(counts, tmp.p, n * N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CDBG_OK;
}

}  // namespace
