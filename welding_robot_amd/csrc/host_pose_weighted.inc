// host_pose_weighted.inc -- C ABI: wa_grid_pose_weighted_fields, wa_grid_pose_weighted_matrix, wa_grid_pose_weighted_paths, cheapest paths
// over (voxel, torch direction) where a step costs hop_cost + turn_cost[class] + pen (included by weldacs.hip inside extern "C", behind
// host_pose.inc, whose checks, keys and setup it uses; the sixth SearchKind of host_geodesic.inc's driver: a ring of R settled sets as for
// host_chamfer_weighted.inc).  The calls are stateless: the masks, the step matrices and the device copy of pen are rebuilt by every call.

// what a call keeps on the device besides pose_prepare's: one adjacency matrix per distinct step weight, the penalty bytes (NULL: none)
struct PosewSetup {
    WaPosewCosts c;
    DevBuf<unsigned long long> adjw;
    DevBuf<uint8_t> pen;
    int32_t top = 0;   // hop_cost + max turn_cost + P: the largest step (R - 1)
};

// rule 30's ranges of the bands and turn costs, and the turn classes dealt over the distinct step weights hop + turn_cost[b] (classes of
// equal cost share a matrix); no device work.  hop is the caller's, already checked (host_pose_diag.inc passes its face step).
static int posew_check_turns(wa_ctx *ctx, const char *who, int32_t hop, int32_t B, const int32_t *turn_band, const int32_t *turn_cost, WaPosewCosts *c)
{
    if (B < 0 || B > WA_POSE_MAX_BANDS) return fail(ctx, WA_ERR_ARG, "%s: n_bands must be 0 .. 4", who);
    for (int32_t b = 0; b < B; b++) {
        if (turn_band[b] < 0 || turn_band[b] > 3 * (1 << 20)) return fail(ctx, WA_ERR_ARG, "%s: a turn band outside 0 .. 3 * 2^20", who);
        if (b && turn_band[b] <= turn_band[b - 1]) return fail(ctx, WA_ERR_ARG, "%s: the turn bands must ascend strictly", who);
    }
    if (turn_cost[0] != 0) return fail(ctx, WA_ERR_ARG, "%s: turn_cost[0] must be 0", who);
    for (int32_t b = 1; b <= B; b++) {
        if (turn_cost[b] > WA_POSE_COST_MAX) return fail(ctx, WA_ERR_ARG, "%s: a turn cost above 15", who);
        if (turn_cost[b] < turn_cost[b - 1]) return fail(ctx, WA_ERR_ARG, "%s: the turn costs must not decrease", who);
    }
    memset(c, 0, sizeof *c);
    c->n_bands = B;
    for (int32_t b = 0; b < B; b++) c->band[b] = turn_band[b];
    for (int32_t b = 0; b <= B; b++) {
        const int32_t w = hop + turn_cost[b];
        if (c->n_w == 0 || c->weight[c->n_w - 1] != w) c->weight[c->n_w++] = w;   // (non-decreasing: equal costs are neighbours)
        c->group[b] = c->n_w - 1;
    }
    return WA_OK;
}

// rule 30's ranges; no device work
static int posew_check(wa_ctx *ctx, const char *who, const wa_pose_costs *costs, WaPosewCosts *c)
{
    if (!costs) return fail(ctx, WA_ERR_ARG, "%s: costs is NULL", who);
    if (costs->hop_cost < 1 || costs->hop_cost > 8) return fail(ctx, WA_ERR_ARG, "%s: hop_cost must be 1 .. 8", who);
    return posew_check_turns(ctx, who, costs->hop_cost, costs->n_bands, costs->turn_band, costs->turn_cost, c);
}

// uploads pen and finds P (WA_ERR_ARG for a byte above 15 on a free voxel), then the step matrices; needs pose_prepare's q on the
// stream.  Nothing has been written to the caller's arrays when this fails.  pen: the caller's bytes (host) or NULL; other_step: the
// largest step that is not a face weight (host_pose_diag.inc's diagonals), which the ring has to hold too.
static int posew_prepare(const wa_grid *g, const char *who, const uint8_t *pen, const PoseSetup &P, PosewSetup &S, int32_t other_step = 0)
{
    wa_ctx *ctx = g->ctx;
    const int64_t n = g->d.n;
    int32_t top_pen = 0;
    if (pen) {
        DevBuf<int32_t> d_info;
        int32_t info[WA_POSEW_PEN_MAX + 2];
        hipError_t e = S.pen.alloc((size_t)n);
        e = e ? e : d_info.alloc((size_t)(WA_POSEW_PEN_MAX + 2));
        if (e != hipSuccess) { (void)hipGetLastError(); hipStreamSynchronize(ctx->stream); return fail(ctx, WA_ERR_ALLOC, "%s: the penalty array does not fit the device", who); }
        e = hipMemcpyAsync(S.pen, pen, (size_t)n, hipMemcpyHostToDevice, ctx->stream);
        e = e ? e : hipMemsetAsync(d_info, 0, sizeof info, ctx->stream);
        if (e == hipSuccess) {
            k_posew_pen_info<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(g->occ, S.pen, n, d_info);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, ctx->stream);
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        e = e ? e : es;
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: checking the penalties: %s", who, hipGetErrorString(e));
        if (info[WA_POSEW_PEN_MAX + 1]) return fail(ctx, WA_ERR_ARG, "%s: a free voxel's penalty is above 15", who);
        for (int32_t q = 1; q <= WA_POSEW_PEN_MAX; q++)
            if (info[q]) top_pen = q;
    }
    S.top = std::max(S.c.weight[S.c.n_w - 1], other_step) + top_pen;
    S.c.R = S.top + 1;
    const int32_t cells = S.c.n_w * P.K * P.W;
    if (S.adjw.alloc((size_t)cells) != hipSuccess) {
        hipStreamSynchronize(ctx->stream);
        return fail(ctx, WA_ERR_ALLOC, "%s: the step matrices", who);
    }
    k_posew_adj<<<(unsigned)((cells + 255) / 256), 256, 0, ctx->stream>>>(P.B.q, P.K, P.max_turn, S.c, S.adjw);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { hipStreamSynchronize(ctx->stream); return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
    return WA_OK;
}

// the ring search over (voxel, direction): `seen` holds every settled state, a source's ring of R settled sets is contiguous and zeroed
// whole, level L reads slots (L - step) mod R and writes slot L mod R whole, and a source is alive while one of the last R - 1 levels
// settled a state.  The field is pose_kind's: n costs and, where states are kept, K * n distances behind them.
static SearchKind posew_kind(const wa_grid *g, const PoseSetup &P, const PosewSetup &S, bool keep_states, const char *fn)
{
    const WaDims gd = g->d;
    const int32_t K = P.K, R = S.c.R;
    SearchKind k;
    k.fn = fn;
    k.frontiers = R; k.zeroed = R; k.window = R - 1;
    k.words = (int64_t)P.W * gd.n; k.ints = gd.n + (keep_states ? (int64_t)K * gd.n : 0);
    // a cheapest path visits a state once: at most K * n_free - 1 steps of at most `top`; R more launches see the ring empty
    k.first = 1; k.bound = std::min<int64_t>((int64_t)S.top * ((int64_t)K * g->n_free - 1) + R + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    hipStream_t st = g->ctx->stream;
    const unsigned long long *open = P.B.mask.p, *adjw = S.adjw.p;
    const uint8_t *pen = S.pen.p;
    const WaPosewCosts c = S.c;
    const int64_t words = k.words, ints = k.ints;
    const int32_t keep = keep_states ? 1 : 0, all_one = P.max_turn < 0 && c.n_w == 1 ? 1 : 0;
    k.seed = [=](const SearchChunk &ch, int32_t ns) {
        k_posew_seed<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(ch.src, ns, open, gd.n, K, R, words, ints, ch.seen, ch.fronts, ch.field, keep, ch.last, ch.stop);
    };
    k.level = [=](const SearchChunk &ch, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        const int32_t nchunk = (gd.nx + 63) / 64;
        const int64_t rows = (int64_t)gd.ny * gd.nz;
        const dim3 grid((unsigned)((int64_t)nchunk * ((rows + 3) / 4)), (unsigned)ns);   // (< 2^28: n <= 2^29)
        const auto kernel = K <= 64 ? k_posew_level<1> : K <= 128 ? k_posew_level<2> : k_posew_level<WA_POSE_MAX_W>;
        kernel<<<grid, 256, 0, st>>>(open, adjw, pen, gd, K, c, all_one, nchunk, (int32_t)level, (int32_t)(level % R), words, ints, ch.seen, ch.fronts,
                                     ch.field, keep, ch.last, ch.stop, d_tgt, n_tgt, ch.mat);
    };
    return k;
}

int wa_grid_pose_weighted_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                 const wa_pose_costs *costs, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *cost_out,
                                 int32_t *state_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_weighted_fields";
    if (!src_ids || !cost_out || n_src < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    PosewSetup S;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : posew_check(ctx, fn, costs, &S.c);
    rc = rc ? rc : pose_check_pins(ctx, fn, src_pin, n_src, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &src_ids, 1, n_src, &d);
    if (rc || n_src == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    rc = rc ? rc : posew_prepare(g, fn, costs->pen, P, S);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(src_ids, src_pin, n_src);
    const SearchKind k = posew_kind(g, P, S, state_out != nullptr, fn);
    const int64_t n = d.n;
    return search_chunks(g, d, k, keys.data(), n_src, true, nullptr, 0, [&](const SearchChunk &c, int32_t s0, int32_t ns) {
        hipError_t e = hipSuccess;
        for (int32_t s = 0; s < ns && e == hipSuccess; s++) {
            const int32_t *f = c.field + (int64_t)s * k.ints;
            e = hipMemcpyAsync(cost_out + (int64_t)(s0 + s) * n, f, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && state_out)
                e = hipMemcpyAsync(state_out + (int64_t)(s0 + s) * K * n, f + n, sizeof(int32_t) * (size_t)((int64_t)K * n), hipMemcpyDeviceToHost, ctx->stream);
        }
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        e = e ? e : es;
        return e == hipSuccess ? (int)WA_OK : fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    });
}

int wa_grid_pose_weighted_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                 const wa_pose_costs *costs, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *cost_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_weighted_matrix";
    if (!point_ids || !cost_out || n_pts < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    PosewSetup S;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : posew_check(ctx, fn, costs, &S.c);
    rc = rc ? rc : pose_check_pins(ctx, fn, point_pin, n_pts, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &point_ids, 1, n_pts, &d);
    if (rc || n_pts == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    rc = rc ? rc : posew_prepare(g, fn, costs->pen, P, S);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(point_ids, point_pin, n_pts);
    return search_rows(g, d, posew_kind(g, P, S, false, fn), keys.data(), n_pts, true, cost_out);
}

int wa_grid_pose_weighted_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                const wa_pose_costs *costs, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                                const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out,
                                int32_t *cost_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_weighted_paths";
    if (!start_ids || !end_ids || !off || !ids_out || !dir_out || !cost_out || !len_out || n_pairs < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    PosewSetup S;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : posew_check(ctx, fn, costs, &S.c);
    rc = rc ? rc : pose_check_pins(ctx, fn, pin_start, n_pairs, K);
    rc = rc ? rc : pose_check_pins(ctx, fn, pin_end, n_pairs, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, fn, start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    rc = rc ? rc : posew_prepare(g, fn, costs->pen, P, S);
    if (rc) return rc;
    const std::vector<int64_t> starts = pose_keys(start_ids, pin_start, n_pairs), ends = pose_keys(end_ids, pin_end, n_pairs);
    const SearchKind k = posew_kind(g, P, S, true, fn);
    // both passes are k_posew_walkback; the writing pass reads what the counting pass left on the device
    DevBuf<int32_t> d_dist, d_kend, d_len;
    PathSteps steps;
    steps.need = "len_out";
    steps.count = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *dist, int32_t *len) {
        hipError_t e = d_dist.alloc((size_t)np);
        e = e ? e : d_kend.alloc((size_t)np);
        e = e ? e : d_len.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_pose_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, k.ints, d.n, K, d_slot, d_end, np, d_dist, d_kend);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        k_posew_walkback<<<(unsigned)np, 64, 0, ctx->stream>>>(c.field, k.ints, g->d, K, S.adjw, S.c, S.pen, d_slot, d_end, nullptr, d_dist, d_kend, np, d_len, nullptr);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(dist, d_dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(len, d_len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        return e ? e : hipStreamSynchronize(ctx->stream);
    };
    steps.write = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_posew_walkback<<<(unsigned)np, 64, 0, ctx->stream>>>(c.field, k.ints, g->d, K, S.adjw, S.c, S.pen, d_slot, d_end, d_dst, d_dist, d_kend, np, d_len, d_out);
        return hipGetLastError();
    };
    rc = search_paths(g, d, k, steps, starts.data(), ends.data(), n_pairs, off, ids_out, cost_out, len_out);
    if (rc != WA_OK && rc != WA_ERR_CAPACITY) return rc;
    // the driver copied each written pair's nodes as keys: the direction index leaves for dir_out, the id stays
    for (int32_t p = 0; p < n_pairs; p++) {
        const int64_t len = len_out[p];
        if (cost_out[p] < 0 || len > off[p + 1] - off[p]) continue;
        for (int64_t i = off[p]; i < off[p] + len; i++) {
            dir_out[i] = (int32_t)(ids_out[i] >> WA_POSE_KEY_SHIFT);
            ids_out[i] = pose_key_id(ids_out[i]);
        }
    }
    return rc;
}
