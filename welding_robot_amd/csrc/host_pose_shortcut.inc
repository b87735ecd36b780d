// host_pose_shortcut.inc -- C ABI: wa_grid_pose_shortcut, the any-angle shortcut of (voxel, direction) paths (included by weldacs.hip
// inside extern "C", behind host_pose.inc, whose argument check it shares, and host_reach.inc, whose k_reach launch gives it the masks:
// the same arena block host_pose.inc searches on).  Stateless like the pose calls: the masks are recomputed by every call.
int wa_grid_pose_shortcut(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *ids,
                          const int32_t *ks, const int64_t *off, int32_t n_paths, int32_t max_span, int64_t *wp_idx, int32_t *hold_out,
                          int32_t *wp_count, double *length_out, wa_pose_shortcut_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_shortcut";
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    if (rc) return rc;
    if (!ids || !ks || !off || !wp_idx || !wp_count || !sum || n_paths < 0 || max_span < 1 || max_span > 4096)
        return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    if (off[0] != 0) return fail(ctx, WA_ERR_ARG, "%s: off[0] != 0", fn);
    for (int32_t p = 0; p < n_paths; p++) {
        if (off[p + 1] < off[p]) return fail(ctx, WA_ERR_ARG, "%s: offsets decrease", fn);
        if (off[p + 1] - off[p] > INT32_MAX) return fail(ctx, WA_ERR_ARG, "%s: a path of 2^31 nodes or more", fn);
    }
    const int64_t N = off[n_paths];
    if (N > ((int64_t)1 << 33)) return fail(ctx, WA_ERR_ARG, "%s: more than 2^33 nodes", fn);
    for (int64_t i = 0; i < N; i++) {
        if (ids[i] < 0 || ids[i] >= g->d.n) return fail(ctx, WA_ERR_ARG, "%s: node id outside the grid", fn);
        if (ks[i] < 0 || ks[i] >= K) return fail(ctx, WA_ERR_ARG, "%s: a direction index outside 0 .. K - 1", fn);
    }
    wa_pose_shortcut_summary s;
    memset(&s, 0, sizeof s);
    s.n_paths = n_paths;
    s.n_nodes = N;
    if (N == 0) {   // only empty paths (or none)
        for (int32_t p = 0; p < n_paths; p++) {
            wp_count[p] = 0;
            if (length_out) length_out[p] = 0.0;
        }
        *sum = s;
        return WA_OK;
    }
    ReachBuffers B(ctx);
    rc = reach_enqueue(g, fn, hq, dt, true, B);
    if (rc) { hipStreamSynchronize(ctx->stream); return rc; }
    hipStream_t st = ctx->stream;
    DevBuf<long long> d_ids, d_off, d_wp;
    DevBuf<int32_t> d_ks, d_step, d_hold, d_hwp, d_cnt;
    DevBuf<double> d_len;
    DevBuf<unsigned long long> d_acc;
    std::vector<long long> wp((size_t)N);
    std::vector<int32_t> hwp(hold_out ? (size_t)N : 0);
    unsigned long long acc[WA_PSC_ACC];
    hipError_t e = d_ids.alloc((size_t)N);
    e = e ? e : d_ks.alloc((size_t)N);
    e = e ? e : d_off.alloc((size_t)n_paths + 1);
    e = e ? e : d_wp.alloc((size_t)N);
    e = e ? e : d_step.alloc((size_t)N);
    e = e ? e : d_hold.alloc((size_t)N);
    e = e ? e : d_hwp.alloc((size_t)N);
    e = e ? e : d_cnt.alloc((size_t)n_paths);
    e = e ? e : d_len.alloc((size_t)n_paths);
    e = e ? e : d_acc.alloc(WA_PSC_ACC);
    if (e != hipSuccess) { hipStreamSynchronize(st); return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", fn); }
    e = hipMemcpyAsync(d_ids, ids, sizeof(long long) * N, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(d_ks, ks, sizeof(int32_t) * N, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(d_off, off, sizeof(long long) * ((size_t)n_paths + 1), hipMemcpyHostToDevice, st);
    e = e ? e : hipMemsetAsync(d_acc, 0, sizeof acc, st);
    if (e == hipSuccess) {
        k_psc_reach<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(d_ids, d_ks, d_off, n_paths, N, max_span, g->d, B.mask.p, B.q, max_turn, d_step, d_hold);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        k_psc_chain<<<(unsigned)((n_paths + 255) / 256), 256, 0, st>>>(d_ids, d_ks, d_off, n_paths, d_step, d_hold, g->d, g->cx, g->cy, g->cz, B.q,
                                                                       d_wp, d_hwp, d_cnt, d_len, d_acc);
        e = hipGetLastError();
    }
    // the counts and lengths go to the caller's arrays only behind a stream that ran clean: staged like the waypoints
    std::vector<int32_t> cnt((size_t)n_paths);
    std::vector<double> len((size_t)n_paths);
    e = e ? e : hipMemcpyAsync(wp.data(), d_wp, sizeof(long long) * N, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && hold_out) e = hipMemcpyAsync(hwp.data(), d_hwp, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st);
    e = e ? e : hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, st);
    e = e ? e : hipMemcpyAsync(len.data(), d_len, sizeof(double) * n_paths, hipMemcpyDeviceToHost, st);
    e = e ? e : hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    e = e ? e : es;
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    // only each path's waypoints: the rest of its range in the caller's buffers stays as it was
    for (int32_t p = 0; p < n_paths; p++) {
        wp_count[p] = cnt[(size_t)p];
        if (length_out) length_out[p] = len[(size_t)p];
        memcpy(wp_idx + off[p], wp.data() + off[p], sizeof(int64_t) * (size_t)cnt[(size_t)p]);
        if (hold_out) memcpy(hold_out + off[p], hwp.data() + off[p], sizeof(int32_t) * (size_t)cnt[(size_t)p]);
    }
    s.n_waypoints = (int64_t)acc[WA_PSC_WAYPOINTS];
    s.n_held_start = (int64_t)acc[WA_PSC_HELD_START];
    s.n_held_end = (int64_t)acc[WA_PSC_HELD_END];
    s.n_unheld = (int64_t)acc[WA_PSC_UNHELD];
    s.max_hold_turn = (int64_t)acc[WA_PSC_MAX_TURN];
    *sum = s;
    return WA_OK;
}
