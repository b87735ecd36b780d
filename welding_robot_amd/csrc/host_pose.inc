// host_pose.inc -- C ABI: wa_grid_pose_fields, wa_grid_pose_matrix, wa_grid_pose_paths, exact paths over (voxel, torch direction) with a
// turn limit (included by weldacs.hip inside extern "C", behind host_geodesic.inc, whose search driver it runs on as a fifth SearchKind,
// and behind host_reach.inc, whose k_reach launch gives it open(v, k)).  The calls are stateless: the masks and the adjacency matrix are
// recomputed by every call.  A source and its pin travel through the driver as one key (pose_kernels.hpp).

// what a call keeps on the device besides the driver's chunk: the masks (a block of the context's arena, inside B), the adjacency matrix
struct PoseSetup {
    ReachBuffers B;
    DevBuf<unsigned long long> adj;
    int32_t K = 0, W = 0, max_turn = -1;
    explicit PoseSetup(wa_ctx *c) : B(c) {}
};

// the arguments the three calls share, behind their NULL checks: rule 16's, then max_turn
static int pose_check(wa_ctx *ctx, const char *who, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                      std::vector<short4> *hq, WaReachTool *dt)
{
    const int rc = reach_check(ctx, who, dirs, K, tool, hq, dt);
    if (rc) return rc;
    if (max_turn < -1 || max_turn > 3 * (1 << 20)) return fail(ctx, WA_ERR_ARG, "%s: max_turn must be -1 or 0 .. 3 * 2^20", who);
    return WA_OK;
}

static int pose_check_pins(wa_ctx *ctx, const char *who, const int32_t *pins, int32_t count, int32_t K)
{
    for (int32_t i = 0; pins && i < count; i++)
        if (pins[i] < -1 || pins[i] >= K) return fail(ctx, WA_ERR_ARG, "%s: a pin outside -1 .. K - 1", who);
    return WA_OK;
}

static std::vector<int64_t> pose_keys(const int64_t *ids, const int32_t *pins, int32_t count)
{
    std::vector<int64_t> keys((size_t)count);
    for (int32_t i = 0; i < count; i++) keys[(size_t)i] = pose_key(ids[i], pins ? pins[i] : -1);
    return keys;
}

// enqueues k_reach (with masks) and k_pose_adj on the context's stream
static int pose_prepare(const wa_grid *g, const char *who, const std::vector<short4> &hq, const WaReachTool &dt, int32_t max_turn, PoseSetup &P)
{
    wa_ctx *ctx = g->ctx;
    P.K = (int32_t)hq.size();
    P.W = (P.K + 63) / 64;
    P.max_turn = max_turn;
    const int rc = reach_enqueue(g, who, hq, dt, true, P.B);
    if (rc) { hipStreamSynchronize(ctx->stream); return rc; }
    if (P.adj.alloc((size_t)P.K * P.W) != hipSuccess) {
        hipStreamSynchronize(ctx->stream);
        return fail(ctx, WA_ERR_ALLOC, "%s: the adjacency matrix", who);
    }
    k_pose_adj<<<(unsigned)((P.K * P.W + 255) / 256), 256, 0, ctx->stream>>>(P.B.q, P.K, max_turn, P.adj);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { hipStreamSynchronize(ctx->stream); return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
    return WA_OK;
}

// breadth-first search over (voxel, direction): bitmaps of W * n words (seen and two frontiers, as for the hop counts), a field of n hop
// counts and, where states are kept, K * n levels behind them
static SearchKind pose_kind(const wa_grid *g, const PoseSetup &P, bool keep_states, const char *fn)
{
    const WaDims gd = g->d;
    const int32_t K = P.K;
    SearchKind k;
    k.fn = fn;
    k.frontiers = 2; k.zeroed = 1; k.window = 1;
    k.words = (int64_t)P.W * gd.n; k.ints = gd.n + (keep_states ? (int64_t)K * gd.n : 0);
    // a search over S <= K * n_free states has at most S - 1 productive levels; one more launch looks at the last frontier
    k.first = 1; k.bound = std::min<int64_t>((int64_t)K * g->n_free + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    hipStream_t st = g->ctx->stream;
    const unsigned long long *open = P.B.mask.p, *adj = P.adj.p;
    const int64_t words = k.words, ints = k.ints;
    const int32_t keep = keep_states ? 1 : 0, all_adj = P.max_turn < 0 ? 1 : 0;
    k.seed = [=](const SearchChunk &c, int32_t ns) {
        k_pose_seed<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(c.src, ns, open, gd.n, K, words, ints, c.seen, c.fronts, c.field, keep, c.last, c.stop);
    };
    k.level = [=](const SearchChunk &c, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        unsigned long long *fa = c.fronts, *fb = c.fronts + (int64_t)c.cap * words;
        const int32_t nchunk = (gd.nx + 63) / 64;
        const int64_t rows = (int64_t)gd.ny * gd.nz;
        const dim3 grid((unsigned)((int64_t)nchunk * ((rows + 3) / 4)), (unsigned)ns);   // (< 2^28: n <= 2^29)
        k_pose_level<<<grid, 256, 0, st>>>(open, adj, gd, K, all_adj, nchunk, (int32_t)level, words, ints, c.seen, (level & 1) ? fa : fb,
                                           (level & 1) ? fb : fa, c.field, keep, c.last, c.stop, d_tgt, n_tgt, c.mat);
    };
    return k;
}

int wa_grid_pose_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *src_ids,
                        const int32_t *src_pin, int32_t n_src, int32_t *hops_out, int32_t *state_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_fields";
    if (!src_ids || !hops_out || n_src < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : pose_check_pins(ctx, fn, src_pin, n_src, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &src_ids, 1, n_src, &d);
    if (rc || n_src == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(src_ids, src_pin, n_src);
    const SearchKind k = pose_kind(g, P, state_out != nullptr, fn);
    const int64_t n = d.n;
    return search_chunks(g, d, k, keys.data(), n_src, true, nullptr, 0, [&](const SearchChunk &c, int32_t s0, int32_t ns) {
        hipError_t e = hipSuccess;
        for (int32_t s = 0; s < ns && e == hipSuccess; s++) {
            const int32_t *f = c.field + (int64_t)s * k.ints;
            e = hipMemcpyAsync(hops_out + (int64_t)(s0 + s) * n, f, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && state_out)
                e = hipMemcpyAsync(state_out + (int64_t)(s0 + s) * K * n, f + n, sizeof(int32_t) * (size_t)((int64_t)K * n), hipMemcpyDeviceToHost, ctx->stream);
        }
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        e = e ? e : es;
        return e == hipSuccess ? (int)WA_OK : fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    });
}

int wa_grid_pose_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *point_ids,
                        const int32_t *point_pin, int32_t n_pts, int32_t *hops_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_matrix";
    if (!point_ids || !hops_out || n_pts < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : pose_check_pins(ctx, fn, point_pin, n_pts, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &point_ids, 1, n_pts, &d);
    if (rc || n_pts == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(point_ids, point_pin, n_pts);
    return search_rows(g, d, pose_kind(g, P, false, fn), keys.data(), n_pts, true, hops_out);
}

int wa_grid_pose_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *start_ids,
                       const int64_t *end_ids, const int32_t *pin_start, const int32_t *pin_end, int32_t n_pairs, const int64_t *off,
                       int64_t *ids_out, int32_t *dir_out, int32_t *hops_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_paths";
    if (!start_ids || !end_ids || !off || !ids_out || !dir_out || !hops_out || n_pairs < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : pose_check_pins(ctx, fn, pin_start, n_pairs, K);
    rc = rc ? rc : pose_check_pins(ctx, fn, pin_end, n_pairs, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, fn, start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    if (rc) return rc;
    const std::vector<int64_t> starts = pose_keys(start_ids, pin_start, n_pairs), ends = pose_keys(end_ids, pin_end, n_pairs);
    const SearchKind k = pose_kind(g, P, true, fn);
    // the writing pass reads the counts and end directions the counting pass left on the device
    DevBuf<int32_t> d_hops, d_kend;
    PathSteps steps;
    steps.need = "hops_out + 1";
    steps.count = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *hops, int32_t *len) {
        hipError_t e = d_hops.alloc((size_t)np);
        e = e ? e : d_kend.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_pose_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, k.ints, d.n, K, d_slot, d_end, np, d_hops, d_kend);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(hops, d_hops, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        for (int32_t i = 0; i < np; i++) len[i] = hops[i] + 1;
        return e;
    };
    steps.write = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_pose_walkback<<<(unsigned)np, 64, 0, ctx->stream>>>(c.field, k.ints, g->d, K, P.adj, d_slot, d_end, d_dst, d_hops, d_kend, np, d_out);
        return hipGetLastError();
    };
    rc = search_paths(g, d, k, steps, starts.data(), ends.data(), n_pairs, off, ids_out, hops_out, len_out);
    if (rc != WA_OK && rc != WA_ERR_CAPACITY) return rc;
    // the driver copied each written pair's nodes as keys: the direction index leaves for dir_out, the id stays
    for (int32_t p = 0; p < n_pairs; p++) {
        const int64_t len = (int64_t)hops_out[p] + 1;
        if (hops_out[p] < 0 || len > off[p + 1] - off[p]) continue;
        for (int64_t i = off[p]; i < off[p] + len; i++) {
            dir_out[i] = (int32_t)(ids_out[i] >> WA_POSE_KEY_SHIFT);
            ids_out[i] = pose_key_id(ids_out[i]);
        }
    }
    return rc;
}
