// host_pose_diag.inc -- C ABI: wa_grid_pose_diag_fields, wa_grid_pose_diag_matrix, wa_grid_pose_diag_paths, cheapest paths over (voxel,
// torch direction) on the 26-neighbour lattice: the face steps of host_pose_weighted.inc plus diagonal moves that keep the direction
// (included by weldacs.hip inside extern "C", behind host_pose_weighted.inc, whose checks, setup and ring it uses; the seventh SearchKind
// of host_geodesic.inc's driver).  The calls are stateless: the masks, the step matrices and the device copy of pen are rebuilt by every
// call.

// rule 43's ranges; the face part becomes a WaPosewCosts with hop = step[0].  No device work.
static int posed_check(wa_ctx *ctx, const char *who, const wa_pose_diag_costs *costs, WaPosewCosts *c)
{
    if (!costs) return fail(ctx, WA_ERR_ARG, "%s: costs is NULL", who);
    for (int i = 0; i < 3; i++)
        if (costs->step[i] < 1 || costs->step[i] > 16) return fail(ctx, WA_ERR_ARG, "%s: every step must be 1 .. 16", who);
    return posew_check_turns(ctx, who, costs->step[0], costs->n_bands, costs->turn_band, costs->turn_cost, c);
}

static int posed_prepare(const wa_grid *g, const char *who, const wa_pose_diag_costs *costs, const PoseSetup &P, PosewSetup &S)
{
    return posew_prepare(g, who, costs->pen, P, S, std::max(costs->step[1], costs->step[2]));
}

// posew_kind with k_posed_level: the same ring (R = S.top + 1 slots, S.top = the largest step plus P), window, fields and bound
static SearchKind posed_kind(const wa_grid *g, const PoseSetup &P, const PosewSetup &S, const wa_pose_diag_costs *costs, bool keep_states, const char *fn)
{
    SearchKind k = posew_kind(g, P, S, keep_states, fn);
    const WaDims gd = g->d;
    const int32_t K = P.K, R = S.c.R;
    hipStream_t st = g->ctx->stream;
    const unsigned long long *open = P.B.mask.p, *adjw = S.adjw.p;
    const uint8_t *pen = S.pen.p;
    WaPosedCosts c;
    c.f = S.c; c.s2 = costs->step[1]; c.s3 = costs->step[2];
    const int32_t keep = keep_states ? 1 : 0, all_one = P.max_turn < 0 && S.c.n_w == 1 ? 1 : 0;
    k.level = [=](const SearchChunk &ch, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        const int32_t nchunk = (gd.nx + 63) / 64;
        const int64_t rows = (int64_t)gd.ny * gd.nz;
        const dim3 grid((unsigned)((int64_t)nchunk * ((rows + 3) / 4)), (unsigned)ns);   // (< 2^28: n <= 2^29)
        const auto kernel = K <= 64 ? k_posed_level<1> : K <= 128 ? k_posed_level<2> : k_posed_level<WA_POSE_MAX_W>;
        kernel<<<grid, 256, 0, st>>>(open, adjw, pen, gd, K, c, all_one, (int32_t)level, (int32_t)(level % R), ch.seen, ch.fronts, ch.field, keep, ch.last,
                                     ch.stop, d_tgt, n_tgt, ch.mat);
    };
    return k;
}

int wa_grid_pose_diag_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                             const wa_pose_diag_costs *costs, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *cost_out,
                             int32_t *state_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_diag_fields";
    if (!src_ids || !cost_out || n_src < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    PosewSetup S;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : posed_check(ctx, fn, costs, &S.c);
    rc = rc ? rc : pose_check_pins(ctx, fn, src_pin, n_src, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &src_ids, 1, n_src, &d);
    if (rc || n_src == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    rc = rc ? rc : posed_prepare(g, fn, costs, P, S);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(src_ids, src_pin, n_src);
    const SearchKind k = posed_kind(g, P, S, costs, state_out != nullptr, fn);
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

int wa_grid_pose_diag_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                             const wa_pose_diag_costs *costs, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *cost_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_diag_matrix";
    if (!point_ids || !cost_out || n_pts < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    PosewSetup S;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : posed_check(ctx, fn, costs, &S.c);
    rc = rc ? rc : pose_check_pins(ctx, fn, point_pin, n_pts, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &point_ids, 1, n_pts, &d);
    if (rc || n_pts == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    rc = rc ? rc : posed_prepare(g, fn, costs, P, S);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(point_ids, point_pin, n_pts);
    return search_rows(g, d, posed_kind(g, P, S, costs, false, fn), keys.data(), n_pts, true, cost_out);
}

int wa_grid_pose_diag_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                            const wa_pose_diag_costs *costs, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                            const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out,
                            int32_t *cost_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_diag_paths";
    if (!start_ids || !end_ids || !off || !ids_out || !dir_out || !cost_out || !len_out || n_pairs < 0) return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    std::vector<short4> hq;
    WaReachTool dt;
    PosewSetup S;
    int rc = pose_check(ctx, fn, dirs, K, tool, max_turn, &hq, &dt);
    rc = rc ? rc : posed_check(ctx, fn, costs, &S.c);
    rc = rc ? rc : pose_check_pins(ctx, fn, pin_start, n_pairs, K);
    rc = rc ? rc : pose_check_pins(ctx, fn, pin_end, n_pairs, K);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, fn, start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare(g, fn, hq, dt, max_turn, P);
    rc = rc ? rc : posed_prepare(g, fn, costs, P, S);
    if (rc) return rc;
    const std::vector<int64_t> starts = pose_keys(start_ids, pin_start, n_pairs), ends = pose_keys(end_ids, pin_end, n_pairs);
    const SearchKind k = posed_kind(g, P, S, costs, true, fn);
    WaPosedCosts c;
    c.f = S.c; c.s2 = costs->step[1]; c.s3 = costs->step[2];
    // both passes are k_posed_walkback; the writing pass reads what the counting pass left on the device
    DevBuf<int32_t> d_dist, d_kend, d_len;
    PathSteps steps;
    steps.need = "len_out";
    steps.count = [&](const SearchChunk &ch, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *dist, int32_t *len) {
        hipError_t e = d_dist.alloc((size_t)np);
        e = e ? e : d_kend.alloc((size_t)np);
        e = e ? e : d_len.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_pose_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(ch.field, k.ints, d.n, K, d_slot, d_end, np, d_dist, d_kend);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        k_posed_walkback<<<(unsigned)np, 64, 0, ctx->stream>>>(ch.field, k.ints, g->d, K, P.B.mask.p, S.adjw, c, S.pen, d_slot, d_end, nullptr, d_dist, d_kend, np, d_len, nullptr);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(dist, d_dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(len, d_len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        return e ? e : hipStreamSynchronize(ctx->stream);
    };
    steps.write = [&](const SearchChunk &ch, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_posed_walkback<<<(unsigned)np, 64, 0, ctx->stream>>>(ch.field, k.ints, g->d, K, P.B.mask.p, S.adjw, c, S.pen, d_slot, d_end, d_dst, d_dist, d_kend, np, d_len, d_out);
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
