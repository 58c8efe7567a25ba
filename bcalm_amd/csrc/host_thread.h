// host_thread.h -- libcdbg.so, host side of cdbg_thread / cdbg_fetch_runs (k_thread.h): the batched walk of a caller's sequences whose hit
// words stay on the device, the run kernels behind each batch, the one comparison per batch seam, and the runs the library keeps for the
// read-out.  Included by cdbg_impl.cpp only.
#pragma once

namespace {

template <int W>
int thread_impl(cdbg_ctx* c, const char* bases, const uint64_t* off, uint64_t n, uint64_t* out) {
    CK(index_refuse(c, "cdbg_thread"));
    out[0] = out[1] = out[2] = out[3] = 0;
    CK(check_offsets("cdbg_thread", off, n));
    thread_forget(c);                                        // (a call that fails leaves no result behind)
    CK(index_impl<W>(c, "cdbg_thread"));
    const uint64_t base0 = n ? off[0] : 0, total = n ? off[n] - base0 : 0;
    hipStream_t s = c->stream;
    const bool marks = HostMarks::enabled();
    float ms_hits = 0, ms_runs = 0;
    if (total) {
        CK(c->th_out.alloc(4, false));
        HIPCK(hipMemsetAsync(c->th_out.p, 0, 4 * sizeof(uint64_t), s));
    }
    // per base of a batch: text + sequence ends + 8 bytes of hits, which stay on the device
    CK(window_batches(c, bases, off, n, [&](uint64_t b0, uint64_t, uint64_t n_out, const WindowParams& wp) -> int {
        // 1. the hit word of every position of the batch, into q_hits
        CK(c->q_hits.alloc(n_out, false));
        ThreadHitParams hp{};
        (WindowParams&)hp = wp; hp.hits = c->q_hits.p; hp.out = c->th_out.p;
        Timer t; if (marks) CK(t.start(s));
        CDBG_LAUNCH((k_thread_hits<W>), (n_out + QUERY_TILE - 1) / QUERY_TILE, QUERY_THREADS, s, hp);
        if (marks) { float ms = 0; CK(t.stop(&ms)); ms_hits += ms; CK(t.start(s)); }
        // 2. heads and tails per tile, their scans, and the batch's runs: the batch's edges are breaks
        const uint64_t tiles = (n_out + THREAD_TILE - 1) / THREAD_TILE;
        CK(c->th_nh.alloc(tiles, false)); CK(c->th_nt.alloc(tiles, false)); CK(c->th_hoff.alloc(tiles + 1, false)); CK(c->th_toff.alloc(tiles + 1, false));
        ThreadRunParams rp{};
        rp.hits = c->q_hits.p; rp.n = n_out; rp.base = b0; rp.n_heads = c->th_nh.p; rp.n_tails = c->th_nt.p;
        CDBG_LAUNCH(k_thread_count, tiles, THREAD_THREADS, s, rp);
        CK(exscan_u32(c, c->th_nh.p, c->th_hoff.p, tiles));
        CK(exscan_u32(c, c->th_nt.p, c->th_toff.p, tiles));
        uint64_t R = 0, Rt = 0;
        CK(read_u64(c->th_hoff.p + tiles, &R)); CK(read_u64(c->th_toff.p + tiles, &Rt));
        if (R != Rt || R > n_out) return fail(CDBG_E_INTERNAL, "cdbg_thread: %llu heads and %llu tails in a batch of %llu positions", (unsigned long long)R, (unsigned long long)Rt, (unsigned long long)n_out);
        const size_t have = c->run_start.size();
        if (R) {                                             // sized from the scanned total, never from the worst case of one run per position
            CK(c->th_start.alloc(R, false)); CK(c->th_place.alloc(R, false)); CK(c->th_tail.alloc(R, false)); CK(c->th_len.alloc(R, false));
            rp.head_off = c->th_hoff.p; rp.tail_off = c->th_toff.p;
            rp.start = c->th_start.p; rp.place = c->th_place.p; rp.tail = c->th_tail.p; rp.len = c->th_len.p; rp.n_runs = R;
            CDBG_LAUNCH(k_thread_emit, tiles, THREAD_THREADS, s, rp);
            CDBG_LAUNCH(k_thread_len, (R + 255) / 256, 256, s, rp);
        }
        if (marks) { float ms = 0; CK(t.stop(&ms)); ms_runs += ms; }
        HIPCK(hipStreamSynchronize(s));                      // (the next batch overwrites the text and the hits)
        HIPCK(hipGetLastError());
        if (R) {
            c->run_start.resize(have + R); c->run_place.resize(have + R); c->run_len.resize(have + R);
            HIPCK(hipMemcpy(c->run_start.data() + have, c->th_start.p, R * sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIPCK(hipMemcpy(c->run_place.data() + have, c->th_place.p, R * sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIPCK(hipMemcpy(c->run_len.data() + have, c->th_len.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost));
            // the seam: the last run before this batch goes on in the batch's first run when the definition says that it continues
            if (have && c->run_start[have] == c->run_start[have - 1] + c->run_len[have - 1]) {
                const uint64_t a = c->run_place[have - 1], steps = (uint64_t)(c->run_len[have - 1] - 1u) << 1;
                if (thread_continues((a & 1) ? a - steps : a + steps, c->run_place[have])) {
                    c->run_len[have - 1] += c->run_len[have];
                    c->run_start.erase(c->run_start.begin() + have); c->run_place.erase(c->run_place.begin() + have); c->run_len.erase(c->run_len.begin() + have);
                }
            }
        }
        return CDBG_OK;
    }));
    uint64_t o[3] = { 0, 0, 0 };
    if (total) CK(read_u64(c->th_out.p, o, 3));
    // the runs of sequence i: those that start inside it (runs lie in position order; no run spans two sequences)
    c->run_off.assign(n + 1, 0);
    const uint64_t R = c->run_start.size();
    uint64_t r = 0;
    for (uint64_t i = 0; i <= n; ++i) {
        const uint64_t lim = n ? off[i] - base0 : 0;
        while (r < R && c->run_start[r] < lim) ++r;
        c->run_off[i] = i == n ? R : r;
    }
    out[0] = o[0]; out[1] = o[1]; out[2] = R; out[3] = o[2];
    c->runs_ready = true;
    if (marks)                                               // dev aid (CDBG_HOST_MARKS=1; bench_micro/thread_timing.py reads it)
        fprintf(stderr, "[thread] positions %llu hits_ms %.3f runs_ms %.3f windows %llu found %llu runs %llu extended %llu\n", (unsigned long long)total, ms_hits, ms_runs,
                (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3]);
    return CDBG_OK;
}

int fetch_runs_impl(cdbg_ctx* c, uint64_t* run_off, uint64_t* start, uint64_t* place, uint32_t* len) {
    CK(index_refuse(c, "cdbg_fetch_runs"));
    if (!c->runs_ready) return fail(CDBG_E_STATE, "cdbg_fetch_runs before cdbg_thread");
    const size_t R = c->run_start.size();
    if (run_off) memcpy(run_off, c->run_off.data(), c->run_off.size() * sizeof(uint64_t));
    if (start && R) memcpy(start, c->run_start.data(), R * sizeof(uint64_t));
    if (place && R) memcpy(place, c->run_place.data(), R * sizeof(uint64_t));
    if (len && R) memcpy(len, c->run_len.data(), R * sizeof(uint32_t));
    return CDBG_OK;
}

}  // namespace
