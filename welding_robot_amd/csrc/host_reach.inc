// host_reach.inc -- C ABI: wa_grid_tool_reach, wa_grid_tool_fit, wa_grid_tool_penalties, the torch-fit planning grids (included by
// weldacs.hip inside extern "C").  The host quantises the directions (rule 1 of the torch section), checks the arguments and works out
// the far-voxel radius; the counts stay on the device, on the context's stream, and feed the follow-up kernels without a read-back.

// floor(sqrt(v)), v >= 0
static int64_t reach_isqrt(int64_t v)
{
    int64_t r = (int64_t)sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

// R^2 of the far-voxel shortcut (DESIGN 4s): R = max over beads of (ceil(dist16 / 16) + 2) + (isqrt(r2) + 1); at most 36 867^2 < 2^31
static uint32_t reach_far2(const WaReachTool &t)
{
#ifdef WA_REACH_NO_PRUNE
    (void)t;
    return 0xffffffffu;   // every free voxel is gathered (tools/reach_time.py measures the shortcut against this build)
#else
    int64_t R = 0;
    for (int32_t j = 0; j < t.n_beads; j++) R = std::max<int64_t>(R, (t.dist16[j] + 15) / 16 + 2 + reach_isqrt((int64_t)t.r2[j]) + 1);
    return (uint32_t)(R * R);
#endif
}

struct ReachBuffers {
    DevBuf<short4> q;
    DevBuf<WaReachTool> tool;
    DevBuf<unsigned long long> rec;
    CtxBuf<unsigned long long> mask;   // W * n words, only when the caller asked for masks
    CtxBuf<uint16_t> count;            // n
    explicit ReachBuffers(wa_ctx *c) : mask(c), count(c) {}
};

// what the three calls share of their arguments: NULL pointers, K, the tool, the directions.  0 or WA_ERR_ARG.
static int reach_check(wa_ctx *ctx, const char *who, const float *dirs, int32_t K, const wa_tool_beads *tool, std::vector<short4> *hq,
                       WaReachTool *dt)
{
    if (!dirs || !tool) return fail(ctx, WA_ERR_ARG, "%s: NULL argument", who);
    if (K < 1 || K > WA_TORCH_MAX_DIRS) return fail(ctx, WA_ERR_ARG, "%s: K must be 1 .. 256", who);
    WaTorchTool tt;
    if (!torch_tool_dev(tool, -1, &tt)) return fail(ctx, WA_ERR_ARG, "%s: n_beads, dist16 or r2 out of range", who);
    memset(dt, 0, sizeof *dt);
    dt->n_beads = tt.n_beads;
    for (int32_t j = 0; j < tt.n_beads; j++) { dt->dist16[j] = tt.dist16[j]; dt->r2[j] = tt.r2[j]; }
    hq->resize((size_t)K);
    for (int32_t k = 0; k < K; k++)
        if (!torch_quantise(dirs + 3 * (size_t)k, &(*hq)[(size_t)k]))
            return fail(ctx, WA_ERR_ARG, "%s: a direction is not finite or has zero length", who);
    return WA_OK;
}

// Enqueues k_reach on the context's stream: B.count (and B.mask when want_mask) hold the result once the stream has got there, B.rec
// the four counters.  The arguments have been checked.
static int reach_enqueue(const wa_grid *g, const char *who, const std::vector<short4> &hq, const WaReachTool &dt, bool want_mask,
                         ReachBuffers &B)
{
    wa_ctx *ctx = g->ctx;
    const int32_t K = (int32_t)hq.size();
    int rc = grid_build_d2(g);
    if (rc) return rc;
    const size_t lds = WA_REACH_LDS_HEAD + (size_t)K * (size_t)dt.n_beads * sizeof(short4);
    if (lds > ((size_t)48 << 10)) {   // (the limit belongs to the function, per device: raised to the most a call can ask for)
        const hipError_t a = hipFuncSetAttribute((const void *)k_reach, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(WA_REACH_LDS_HEAD + WA_TORCH_MAX_DIRS * WA_TORCH_MAX_BEADS * sizeof(short4)));
        if (a != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: dynamic LDS limit: %s", who, hipGetErrorString(a));
    }
    const int64_t n = g->d.n;
    const size_t W = (size_t)((K + 63) / 64);
    hipError_t e = B.q.alloc((size_t)K);
    e = e ? e : B.tool.alloc(1);
    e = e ? e : B.rec.alloc(4);
    e = e ? e : B.count.alloc((size_t)n);
    if (want_mask) e = e ? e : B.mask.alloc(W * (size_t)n);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", who);
    hipStream_t st = ctx->stream;
    e = hipMemcpyAsync(B.q, hq.data(), sizeof(short4) * (size_t)K, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(B.tool, &dt, sizeof dt, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemsetAsync(B.rec, 0, 4 * sizeof(unsigned long long), st);
    if (e == hipSuccess) {
        const int32_t nchunk = (g->d.nx + 63) / 64;
        const int64_t rows = (int64_t)g->d.ny * g->d.nz;
        const int64_t blocks = (int64_t)nchunk * ((rows + 3) / 4);   // (< 2^28: n <= 2^29)
        k_reach<<<(unsigned)blocks, 256, lds, st>>>(g->occ, g->d2, g->d, B.q, K, B.tool, reach_far2(dt), nchunk, want_mask ? B.mask.p : nullptr,
                                                    B.count, B.rec);
        e = hipGetLastError();
    }
    // (hq and dt are the caller's and outlive the copies: every caller synchronises the stream before it returns)
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return WA_OK;
}

static void reach_summary_from(const unsigned long long rec[4], wa_reach_summary *s)
{
    s->n_free = (int64_t)rec[0];
    s->n_no_dir = (int64_t)rec[1];
    s->n_all_dirs = (int64_t)rec[2];
    s->n_blocked_pairs = (int64_t)rec[3];
}

int wa_grid_tool_reach(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, uint64_t *mask_out, uint16_t *count_out,
                       wa_reach_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!sum) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_reach: NULL argument");
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = reach_check(ctx, "wa_grid_tool_reach", dirs, K, tool, &hq, &dt);
    if (rc) return rc;
    ReachBuffers B(ctx);
    rc = reach_enqueue(g, "wa_grid_tool_reach", hq, dt, mask_out != nullptr, B);
    if (rc) { hipStreamSynchronize(ctx->stream); return rc; }
    const size_t n = (size_t)g->d.n, W = (size_t)((K + 63) / 64);
    unsigned long long rec[4];
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(rec, B.rec, sizeof rec, hipMemcpyDeviceToHost, st);
    if (mask_out) e = e ? e : hipMemcpyAsync(mask_out, B.mask, sizeof(uint64_t) * W * n, hipMemcpyDeviceToHost, st);
    if (count_out) e = e ? e : hipMemcpyAsync(count_out, B.count, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) { hipStreamSynchronize(st); return fail(ctx, WA_ERR_DEVICE, "wa_grid_tool_reach: %s", hipGetErrorString(e)); }
    reach_summary_from(rec, sum);
    return WA_OK;
}

int wa_grid_tool_fit(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t min_dirs, const int64_t *keep_ids,
                     int32_t n_keep, int32_t keep_r2, wa_grid **out, wa_reach_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!out || (n_keep > 0 && !keep_ids)) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_fit: NULL argument");
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = reach_check(ctx, "wa_grid_tool_fit", dirs, K, tool, &hq, &dt);
    if (rc) return rc;
    if (min_dirs < 1 || min_dirs > K) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_fit: min_dirs must be 1 .. K");
    if (n_keep < 0) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_fit: negative number of keep ids");
    if (keep_r2 < 0 || keep_r2 > (1 << 30)) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_fit: keep_r2 must be 0 .. 2^30");
    for (int32_t k = 0; k < n_keep; k++)
        if (keep_ids[k] < 0 || keep_ids[k] >= g->d.n) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_fit: keep id outside the grid");
    if (n_keep > 0) {
        std::vector<uint8_t> keep_free((size_t)n_keep);
        for (int32_t k = 0; k < n_keep; k++) HIPC(ctx, hipMemcpy(&keep_free[(size_t)k], g->occ + keep_ids[k], 1, hipMemcpyDeviceToHost));
        for (int32_t k = 0; k < n_keep; k++)
            if (!keep_free[(size_t)k]) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_fit: keep id is not a free voxel");
    }
    std::vector<float> ax[3] = {std::vector<float>((size_t)g->d.nx), std::vector<float>((size_t)g->d.ny), std::vector<float>((size_t)g->d.nz)};
    rc = wa_grid_read_coords(g, ax[0].data(), ax[1].data(), ax[2].data());
    if (rc) return rc;
    wa_grid *ng = nullptr;
    rc = grid_alloc(ctx, g->d.nx, g->d.ny, g->d.nz, ax[0].data(), ax[1].data(), ax[2].data(), g->precision, g->wall, &ng);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    unsigned long long rec[4] = {0, 0, 0, 0};
    {
        ReachBuffers B(ctx);   // (its destructor waits for the stream: nothing below leaves a kernel running on freed blocks)
        DevBuf<long long> d_keep;
        rc = reach_enqueue(g, "wa_grid_tool_fit", hq, dt, false, B);
        hipError_t e = hipSuccess;
        if (rc == WA_OK) {
            k_reach_fit<<<2048, 256, 0, st>>>(g->occ, B.count, g->d.n, min_dirs, ng->occ);
            e = hipGetLastError();
            if (e == hipSuccess && n_keep > 0) {
                e = d_keep.alloc((size_t)n_keep);
                e = e ? e : hipMemcpyAsync(d_keep, keep_ids, sizeof(long long) * (size_t)n_keep, hipMemcpyHostToDevice, st);
                if (e == hipSuccess) {
                    // half-width of the bubble's box, capped by the grid: |v - k|^2 <= keep_r2 needs every |v_c - k_c| <= isqrt(keep_r2)
                    const int32_t h = (int32_t)std::min<int64_t>(reach_isqrt(keep_r2), std::max(g->d.nx, std::max(g->d.ny, g->d.nz)));
                    k_reach_keep<<<(unsigned)n_keep, 256, 0, st>>>(g->occ, g->d, d_keep, h, (int64_t)keep_r2, ng->occ);
                    e = hipGetLastError();
                }
            }
            e = e ? e : hipMemcpyAsync(rec, B.rec, sizeof rec, hipMemcpyDeviceToHost, st);
        }
        const hipError_t es = hipStreamSynchronize(st);
        e = e ? e : es;
        if (rc == WA_OK && e != hipSuccess) rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_tool_fit: %s", hipGetErrorString(e));
    }
    rc = rc ? rc : grid_count_free(ng);
    if (rc) { wa_grid_destroy(ng); return rc; }
    if (sum) reach_summary_from(rec, sum);
    *out = ng;
    return WA_OK;
}

int wa_grid_tool_penalties(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, const int32_t *thr, int32_t n_thr,
                           uint8_t *pen_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!pen_out || (n_thr > 0 && !thr)) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_penalties: NULL argument");
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = reach_check(ctx, "wa_grid_tool_penalties", dirs, K, tool, &hq, &dt);
    if (rc) return rc;
    if (n_thr < 0 || n_thr > WA_PEN_MAX) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_penalties: n_thr must be 0 .. WA_PEN_MAX");
    WaReachThr T;
    memset(&T, 0, sizeof T);
    T.n = n_thr;
    for (int32_t t = 0; t < n_thr; t++) {
        if (thr[t] < 0 || thr[t] > 65535) return fail(ctx, WA_ERR_ARG, "wa_grid_tool_penalties: a threshold must be 0 .. 65535");
        T.thr[t] = thr[t];
    }
    ReachBuffers B(ctx);
    DevBuf<uint8_t> d_pen;
    rc = reach_enqueue(g, "wa_grid_tool_penalties", hq, dt, false, B);
    if (rc) { hipStreamSynchronize(ctx->stream); return rc; }
    hipStream_t st = ctx->stream;
    hipError_t e = d_pen.alloc((size_t)g->d.n);
    if (e != hipSuccess) { hipStreamSynchronize(st); return fail(ctx, WA_ERR_ALLOC, "wa_grid_tool_penalties: device buffers"); }
    k_reach_penalties<<<2048, 256, 0, st>>>(g->occ, B.count, g->d.n, T, d_pen);
    e = hipGetLastError();
    e = e ? e : hipMemcpyAsync(pen_out, d_pen, (size_t)g->d.n, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    e = e ? e : es;
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_tool_penalties: %s", hipGetErrorString(e));
    return WA_OK;
}
