// host_shortcut.inc -- C ABI: any-angle shortening of planned paths by line of sight (included by weldacs.hip inside extern "C")
int wa_grid_path_shortcut(const wa_grid *g, const int64_t *ids, const int64_t *off, int32_t n_paths, int32_t max_span,
                          int64_t *wp_idx, int32_t *wp_count, double *length_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!ids || !off || !wp_idx || !wp_count || n_paths < 0 || max_span < 1 || max_span > 4096)
        return fail(ctx, WA_ERR_ARG, "wa_grid_path_shortcut: bad argument");
    if (off[0] != 0) return fail(ctx, WA_ERR_ARG, "wa_grid_path_shortcut: off[0] != 0");
    for (int32_t p = 0; p < n_paths; p++) {
        if (off[p + 1] < off[p]) return fail(ctx, WA_ERR_ARG, "wa_grid_path_shortcut: offsets decrease");
        if (off[p + 1] - off[p] > INT32_MAX) return fail(ctx, WA_ERR_ARG, "wa_grid_path_shortcut: a path of 2^31 nodes or more");
    }
    const int64_t N = off[n_paths];
    if (N > ((int64_t)1 << 33)) return fail(ctx, WA_ERR_ARG, "wa_grid_path_shortcut: more than 2^33 nodes");
    for (int64_t i = 0; i < N; i++)
        if (ids[i] < 0 || ids[i] >= g->d.n) return fail(ctx, WA_ERR_ARG, "wa_grid_path_shortcut: node id outside the grid");
    if (N == 0) {   // only empty paths (or none)
        for (int32_t p = 0; p < n_paths; p++) {
            wp_count[p] = 0;
            if (length_out) length_out[p] = 0.0;
        }
        return WA_OK;
    }
    DevBuf<long long> d_ids, d_off, d_wp;
    DevBuf<int32_t> d_step, d_cnt;
    DevBuf<double> d_len;
    std::vector<long long> wp((size_t)N);
    hipError_t e = d_ids.alloc((size_t)N);
    e = e ? e : d_off.alloc((size_t)n_paths + 1);
    e = e ? e : d_wp.alloc((size_t)N);
    e = e ? e : d_step.alloc((size_t)N);
    e = e ? e : d_cnt.alloc((size_t)n_paths);
    e = e ? e : d_len.alloc((size_t)n_paths);
    e = e ? e : hipMemcpyAsync(d_ids, ids, sizeof(long long) * N, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(d_off, off, sizeof(long long) * ((size_t)n_paths + 1), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        k_sc_reach<<<(unsigned)((N + 3) / 4), 256, 0, ctx->stream>>>(d_ids, d_off, n_paths, N, max_span, g->d, g->occ, d_step);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        k_sc_chain<<<(unsigned)((n_paths + 255) / 256), 256, 0, ctx->stream>>>(d_ids, d_off, n_paths, d_step, g->d, g->cx, g->cy, g->cz,
                                                                             d_wp, d_cnt, d_len);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(wp.data(), d_wp, sizeof(long long) * N, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipMemcpyAsync(wp_count, d_cnt, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && length_out) e = hipMemcpyAsync(length_out, d_len, sizeof(double) * n_paths, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_path_shortcut: %s", hipGetErrorString(e));
    // only each path's waypoints: the rest of its range in the caller's buffer stays as it was
    for (int32_t p = 0; p < n_paths; p++)
        memcpy(wp_idx + off[p], wp.data() + off[p], sizeof(int64_t) * (size_t)wp_count[p]);
    return WA_OK;
}
