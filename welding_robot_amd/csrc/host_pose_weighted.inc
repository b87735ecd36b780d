// host_pose_weighted.inc -- C ABI: the two cost flavours of the pose family (included by weldacs.hip inside extern "C", behind
// host_pose.inc, whose three call shapes they run on).  wa_grid_pose_weighted_fields / _matrix / _paths: cheapest paths over (voxel,
// torch direction) where a step costs hop_cost + turn_cost[class] + pen.  wa_grid_pose_diag_fields / _matrix / _paths: the same on the
// 26-neighbour lattice, face steps of step[0] plus diagonal moves that keep the direction.  Both are one ring search (a ring of R
// settled sets as for host_chamfer.inc's weighted calls, pose_weighted_kernels.hpp), told apart by the lattice: posew_kind and posew_steps take
// it as a parameter.  The calls are stateless: the masks, the step matrices and the device copy of pen are rebuilt by every call.

// what a call keeps on the device besides pose_prepare's: one adjacency matrix per distinct face weight, the penalty bytes (NULL: none)
struct PosewSetup {
    WaPosewCosts c;
    const uint8_t *host_pen = nullptr;   // the caller's penalties, or NULL (set by the cost check)
    DevBuf<unsigned long long> adjw;
    DevBuf<uint8_t> pen;
    int32_t top = 0;   // the largest step plus P (R - 1)
};

// rule 30's ranges of the bands and turn costs, and the turn classes dealt over the distinct step weights hop + turn_cost[b] (classes of
// equal cost share a matrix); no device work.  hop is the caller's, already checked (hop_cost, or the face step of the 26 neighbours).
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
static int posew_check(wa_ctx *ctx, const char *who, const wa_pose_costs *costs, PosewSetup *S)
{
    if (!costs) return fail(ctx, WA_ERR_ARG, "%s: costs is NULL", who);
    if (costs->hop_cost < 1 || costs->hop_cost > 8) return fail(ctx, WA_ERR_ARG, "%s: hop_cost must be 1 .. 8", who);
    S->host_pen = costs->pen;
    return posew_check_turns(ctx, who, costs->hop_cost, costs->n_bands, costs->turn_band, costs->turn_cost, &S->c);
}

// rule 43's ranges; the face part is posew_check's with hop = step[0], the diagonal steps follow it.  No device work.
static int posed_check(wa_ctx *ctx, const char *who, const wa_pose_diag_costs *costs, PosewSetup *S)
{
    if (!costs) return fail(ctx, WA_ERR_ARG, "%s: costs is NULL", who);
    for (int i = 0; i < 3; i++)
        if (costs->step[i] < 1 || costs->step[i] > 16) return fail(ctx, WA_ERR_ARG, "%s: every step must be 1 .. 16", who);
    S->host_pen = costs->pen;
    const int rc = posew_check_turns(ctx, who, costs->step[0], costs->n_bands, costs->turn_band, costs->turn_cost, &S->c);
    S->c.s2 = costs->step[1];   // (behind posew_check_turns, which clears the description)
    S->c.s3 = costs->step[2];
    return rc;
}

// uploads pen and finds P (WA_ERR_ARG for a byte above 15 on a free voxel), then the step matrices; needs pose_prepare's q on the
// stream.  Nothing has been written to the caller's arrays when this fails.  The ring has to hold the largest step, a face weight or
// a diagonal step (0 on the face lattice).
static int posew_prepare(const wa_grid *g, const char *who, const PoseSetup &P, PosewSetup &S)
{
    wa_ctx *ctx = g->ctx;
    const int64_t n = g->d.n;
    const uint8_t *pen = S.host_pen;
    const int32_t other_step = std::max(S.c.s2, S.c.s3);
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

// the ring search over (voxel, direction), diag: on the 26-neighbour lattice.  `seen` holds every settled state, a source's ring of R
// settled sets is contiguous and zeroed whole, level L reads slots (L - step) mod R and writes slot L mod R whole, and a source is alive
// while one of the last R - 1 levels settled a state.  The field is pose_kind's: n costs and, where states are kept, K * n distances
// behind them.
static SearchKind posew_kind(const wa_grid *g, const PoseSetup &P, const PosewSetup &S, bool diag, bool keep_states, const char *fn)
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
        // K picks the planes the registers hold, for both lattices; the lattice picks the instantiation
        const auto kernel = K <= 64 ? k_posew_level<1> : K <= 128 ? k_posew_level<2> : k_posew_level<WA_POSE_MAX_W>;
        kernel[diag ? 1 : 0]<<<grid, 256, 0, st>>>(open, adjw, pen, gd, K, c, all_one, (int32_t)level, (int32_t)(level % R), ch.seen, ch.fronts, ch.field, keep,
                                                   ch.last, ch.stop, d_tgt, n_tgt, ch.mat, nchunk, words, ints);
    };
    return k;
}

// the ring search's passes: k_pose_pair_hops, then k_posew_walkback twice -- the counting pass, whose counts and distances go to the
// host, and the writing pass, which reads what the counting pass left on the device
static PathSteps posew_steps(const wa_grid *g, const PoseSetup &P, const PosewSetup &S, bool diag, const SearchKind &k, PosePathBufs &b)
{
    hipStream_t st = g->ctx->stream;
    const WaDims gd = g->d;
    const int32_t K = P.K;
    const int64_t ints = k.ints;
    const unsigned long long *open = P.B.mask.p, *adjw = S.adjw.p;
    const uint8_t *pen = S.pen.p;
    const WaPosewCosts c = S.c;
    const auto walkback = diag ? k_posew_walkback<true> : k_posew_walkback<false>;
    PathSteps steps;
    steps.need = "len_out";
    steps.count = [=, &b](const SearchChunk &ch, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *dist, int32_t *len) {
        hipError_t e = b.dist.alloc((size_t)np);
        e = e ? e : b.kend.alloc((size_t)np);
        e = e ? e : b.len.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_pose_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(ch.field, ints, gd.n, K, d_slot, d_end, np, b.dist, b.kend);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        walkback<<<(unsigned)np, 64, 0, st>>>(ch.field, ints, gd, K, open, adjw, c, pen, d_slot, d_end, nullptr, b.dist, b.kend, np, b.len, nullptr);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(dist, b.dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st);
        e = e ? e : hipMemcpyAsync(len, b.len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st);
        return e ? e : hipStreamSynchronize(st);
    };
    steps.write = [=, &b](const SearchChunk &ch, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        walkback<<<(unsigned)np, 64, 0, st>>>(ch.field, ints, gd, K, open, adjw, c, pen, d_slot, d_end, d_dst, b.dist, b.kend, np, b.len, d_out);
        return hipGetLastError();
    };
    return steps;
}

// a cost flavour: check is posew_check or posed_check on the caller's description, filling S
static PoseFlavour posew_flavour(const PoseArgs &a, PosewSetup &S, bool diag, std::function<int()> check)
{
    PoseFlavour f;
    f.check = std::move(check);
    f.prepare = [&a, &S](const PoseSetup &P) { return posew_prepare(a.g, a.fn, P, S); };
    f.kind = [&a, &S, diag](const PoseSetup &P, bool keep_states) { return posew_kind(a.g, P, S, diag, keep_states, a.fn); };
    f.steps = [&a, &S, diag](const PoseSetup &P, const SearchKind &k, PosePathBufs &b) { return posew_steps(a.g, P, S, diag, k, b); };
    f.len_is_given = true;
    return f;
}
static PoseFlavour posew_weighted(const PoseArgs &a, PosewSetup &S, const wa_pose_costs *costs)
{
    return posew_flavour(a, S, false, [&a, &S, costs] { return posew_check(a.g->ctx, a.fn, costs, &S); });
}
static PoseFlavour posew_diagonal(const PoseArgs &a, PosewSetup &S, const wa_pose_diag_costs *costs)
{
    return posew_flavour(a, S, true, [&a, &S, costs] { return posed_check(a.g->ctx, a.fn, costs, &S); });
}

int wa_grid_pose_weighted_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                 const wa_pose_costs *costs, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *cost_out,
                                 int32_t *state_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_weighted_fields", dirs, K, tool, max_turn};
    if (!src_ids || !cost_out || n_src < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    PosewSetup S;
    return pose_fields(a, posew_weighted(a, S, costs), src_ids, src_pin, n_src, cost_out, state_out);
}

int wa_grid_pose_weighted_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                 const wa_pose_costs *costs, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *cost_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_weighted_matrix", dirs, K, tool, max_turn};
    if (!point_ids || !cost_out || n_pts < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    PosewSetup S;
    return pose_matrix(a, posew_weighted(a, S, costs), point_ids, point_pin, n_pts, cost_out);
}

int wa_grid_pose_weighted_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                const wa_pose_costs *costs, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                                const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out,
                                int32_t *cost_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_weighted_paths", dirs, K, tool, max_turn};
    if (!start_ids || !end_ids || !off || !ids_out || !dir_out || !cost_out || !len_out || n_pairs < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    PosewSetup S;
    return pose_paths(a, posew_weighted(a, S, costs), start_ids, end_ids, pin_start, pin_end, n_pairs, off, ids_out, dir_out, cost_out, len_out);
}

int wa_grid_pose_diag_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                             const wa_pose_diag_costs *costs, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *cost_out,
                             int32_t *state_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_diag_fields", dirs, K, tool, max_turn};
    if (!src_ids || !cost_out || n_src < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    PosewSetup S;
    return pose_fields(a, posew_diagonal(a, S, costs), src_ids, src_pin, n_src, cost_out, state_out);
}

int wa_grid_pose_diag_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                             const wa_pose_diag_costs *costs, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *cost_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_diag_matrix", dirs, K, tool, max_turn};
    if (!point_ids || !cost_out || n_pts < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    PosewSetup S;
    return pose_matrix(a, posew_diagonal(a, S, costs), point_ids, point_pin, n_pts, cost_out);
}

int wa_grid_pose_diag_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                            const wa_pose_diag_costs *costs, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                            const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out,
                            int32_t *cost_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_diag_paths", dirs, K, tool, max_turn};
    if (!start_ids || !end_ids || !off || !ids_out || !dir_out || !cost_out || !len_out || n_pairs < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    PosewSetup S;
    return pose_paths(a, posew_diagonal(a, S, costs), start_ids, end_ids, pin_start, pin_end, n_pairs, off, ids_out, dir_out, cost_out, len_out);
}
