// host_pose.inc -- the pose family: exact paths over (voxel, torch direction) with a turn limit (included by weldacs.hip inside
// extern "C", behind host_geodesic.inc, whose search driver it runs on, and behind host_reach.inc, whose k_reach launch gives it
// open(v, k)).  The family has three call shapes, _fields, _matrix and _paths, in three flavours: hop counts (wa_grid_pose_*, this file),
// turn costs and diagonal moves (wa_grid_pose_weighted_* and wa_grid_pose_diag_*, host_pose_weighted.inc).  pose_fields, pose_matrix and
// pose_paths below run a shape once for all flavours; a PoseFlavour says what is the flavour's own.  The calls are stateless: the masks
// and the adjacency matrix are recomputed by every call.  A source and its pin travel through the driver as one key (pose_kernels.hpp).

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

// what the exported calls share behind their own NULL checks
struct PoseArgs {
    const wa_grid *g;
    const char *fn;   // the exported function, in front of every message
    const float *dirs;
    int32_t K;
    const wa_tool_beads *tool;
    int32_t max_turn;
};

// what the writing pass of a _paths call reads of its counting pass, on the device
struct PosePathBufs {
    DevBuf<int32_t> dist, kend, len;
};

// What tells one flavour from another.  check and prepare may be empty (hop counts).
struct PoseFlavour {
    std::function<int()> check;                            // the cost description's ranges, between pose_check and the pins; no device work
    std::function<int(const PoseSetup &)> prepare;         // what follows pose_prepare on the stream
    std::function<SearchKind(const PoseSetup &, bool)> kind;                                   // (P, keep_states)
    std::function<PathSteps(const PoseSetup &, const SearchKind &, PosePathBufs &)> steps;     // _paths: the two passes
    bool len_is_given;    // _paths: a pair's node count is len_out[p] (which the call requires); else hops + 1, and len_out may be NULL
};

// the checks every shape starts with: rule 16's and max_turn, the flavour's costs, the pins (pins_b: the second list of a _paths call)
static int pose_check_all(const PoseArgs &a, const PoseFlavour &f, const int32_t *pins_a, const int32_t *pins_b, int32_t count,
                          std::vector<short4> *hq, WaReachTool *dt)
{
    wa_ctx *ctx = a.g->ctx;
    int rc = pose_check(ctx, a.fn, a.dirs, a.K, a.tool, a.max_turn, hq, dt);
    if (rc == WA_OK && f.check) rc = f.check();
    rc = rc ? rc : pose_check_pins(ctx, a.fn, pins_a, count, a.K);
    rc = rc ? rc : pose_check_pins(ctx, a.fn, pins_b, count, a.K);
    return rc;
}

// pose_prepare, then the flavour's own step
static int pose_prepare_all(const PoseArgs &a, const PoseFlavour &f, const std::vector<short4> &hq, const WaReachTool &dt, PoseSetup &P)
{
    const int rc = pose_prepare(a.g, a.fn, hq, dt, a.max_turn, P);
    return rc == WA_OK && f.prepare ? f.prepare(P) : rc;
}

// a _fields call behind its NULL checks: out takes a row of n per source, state_out (or NULL) K rows of n per source
static int pose_fields(const PoseArgs &a, const PoseFlavour &f, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *out,
                       int32_t *state_out)
{
    const wa_grid *g = a.g;
    wa_ctx *ctx = g->ctx;
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check_all(a, f, src_pin, nullptr, n_src, &hq, &dt);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, a.fn, &src_ids, 1, n_src, &d);
    if (rc || n_src == 0) return rc;
    PoseSetup P(ctx);
    rc = pose_prepare_all(a, f, hq, dt, P);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(src_ids, src_pin, n_src);
    const SearchKind k = f.kind(P, state_out != nullptr);
    const int64_t n = d.n;
    const int32_t K = P.K;
    return search_chunks(g, d, k, keys.data(), n_src, true, nullptr, 0, [&](const SearchChunk &c, int32_t s0, int32_t ns) {
        hipError_t e = hipSuccess;
        for (int32_t s = 0; s < ns && e == hipSuccess; s++) {
            const int32_t *fld = c.field + (int64_t)s * k.ints;
            e = hipMemcpyAsync(out + (int64_t)(s0 + s) * n, fld, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && state_out)
                e = hipMemcpyAsync(state_out + (int64_t)(s0 + s) * K * n, fld + n, sizeof(int32_t) * (size_t)((int64_t)K * n), hipMemcpyDeviceToHost, ctx->stream);
        }
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        e = e ? e : es;
        return e == hipSuccess ? (int)WA_OK : fail(ctx, WA_ERR_DEVICE, "%s: %s", a.fn, hipGetErrorString(e));
    });
}

// a _matrix call behind its NULL checks
static int pose_matrix(const PoseArgs &a, const PoseFlavour &f, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *out)
{
    const wa_grid *g = a.g;
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check_all(a, f, point_pin, nullptr, n_pts, &hq, &dt);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, a.fn, &point_ids, 1, n_pts, &d);
    if (rc || n_pts == 0) return rc;
    PoseSetup P(g->ctx);
    rc = pose_prepare_all(a, f, hq, dt, P);
    if (rc) return rc;
    const std::vector<int64_t> keys = pose_keys(point_ids, point_pin, n_pts);
    return search_rows(g, d, f.kind(P, false), keys.data(), n_pts, true, out);
}

// a _paths call behind its NULL checks
static int pose_paths(const PoseArgs &a, const PoseFlavour &f, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                      const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out, int32_t *dist_out,
                      int32_t *len_out)
{
    const wa_grid *g = a.g;
    std::vector<short4> hq;
    WaReachTool dt;
    int rc = pose_check_all(a, f, pin_start, pin_end, n_pairs, &hq, &dt);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, a.fn, start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    PoseSetup P(g->ctx);
    rc = pose_prepare_all(a, f, hq, dt, P);
    if (rc) return rc;
    const std::vector<int64_t> starts = pose_keys(start_ids, pin_start, n_pairs), ends = pose_keys(end_ids, pin_end, n_pairs);
    const SearchKind k = f.kind(P, true);
    PosePathBufs bufs;
    const PathSteps steps = f.steps(P, k, bufs);
    rc = search_paths(g, d, k, steps, starts.data(), ends.data(), n_pairs, off, ids_out, dist_out, len_out);
    if (rc != WA_OK && rc != WA_ERR_CAPACITY) return rc;
    // the driver copied each written pair's nodes as keys: the direction index leaves for dir_out, the id stays
    for (int32_t p = 0; p < n_pairs; p++) {
        const int64_t len = f.len_is_given ? (int64_t)len_out[p] : (int64_t)dist_out[p] + 1;
        if (dist_out[p] < 0 || len > off[p + 1] - off[p]) continue;
        for (int64_t i = off[p]; i < off[p] + len; i++) {
            dir_out[i] = (int32_t)(ids_out[i] >> WA_POSE_KEY_SHIFT);
            ids_out[i] = pose_key_id(ids_out[i]);
        }
    }
    return rc;
}

// breadth-first search over (voxel, direction): bitmaps of W * n words (seen and two frontiers, as for the hop counts), a field of n hop
// counts and, where states are kept, K * n levels behind them.  The seed is the ring's with R = 1: source s's first frontier.
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
        k_posew_seed<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(c.src, ns, open, gd.n, K, 1, words, ints, c.seen, c.fronts, c.field, keep, c.last, c.stop);
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

// the hop counts' passes: a path has hops + 1 nodes, so the counting pass is k_pose_pair_hops alone
static PathSteps pose_steps(const wa_grid *g, const PoseSetup &P, const SearchKind &k, PosePathBufs &b)
{
    hipStream_t st = g->ctx->stream;
    const WaDims gd = g->d;
    const int32_t K = P.K;
    const int64_t ints = k.ints;
    const unsigned long long *adj = P.adj.p;
    PathSteps steps;
    steps.need = "hops_out + 1";
    steps.count = [=, &b](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *hops, int32_t *len) {
        hipError_t e = b.dist.alloc((size_t)np);
        e = e ? e : b.kend.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_pose_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(c.field, ints, gd.n, K, d_slot, d_end, np, b.dist, b.kend);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(hops, b.dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        for (int32_t i = 0; i < np; i++) len[i] = hops[i] + 1;
        return e;
    };
    steps.write = [=, &b](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_pose_walkback<<<(unsigned)np, 64, 0, st>>>(c.field, ints, gd, K, adj, d_slot, d_end, d_dst, b.dist, b.kend, np, d_out);
        return hipGetLastError();
    };
    return steps;
}

// hop counts: no costs to check, nothing to prepare beyond pose_prepare
static PoseFlavour pose_hops(const PoseArgs &a)
{
    PoseFlavour f;
    f.kind = [&a](const PoseSetup &P, bool keep_states) { return pose_kind(a.g, P, keep_states, a.fn); };
    f.steps = [&a](const PoseSetup &P, const SearchKind &k, PosePathBufs &b) { return pose_steps(a.g, P, k, b); };
    f.len_is_given = false;
    return f;
}

int wa_grid_pose_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *src_ids,
                        const int32_t *src_pin, int32_t n_src, int32_t *hops_out, int32_t *state_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_fields", dirs, K, tool, max_turn};
    if (!src_ids || !hops_out || n_src < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    return pose_fields(a, pose_hops(a), src_ids, src_pin, n_src, hops_out, state_out);
}

int wa_grid_pose_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *point_ids,
                        const int32_t *point_pin, int32_t n_pts, int32_t *hops_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_matrix", dirs, K, tool, max_turn};
    if (!point_ids || !hops_out || n_pts < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);
    return pose_matrix(a, pose_hops(a), point_ids, point_pin, n_pts, hops_out);
}

int wa_grid_pose_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *start_ids,
                       const int64_t *end_ids, const int32_t *pin_start, const int32_t *pin_end, int32_t n_pairs, const int64_t *off,
                       int64_t *ids_out, int32_t *dir_out, int32_t *hops_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    const PoseArgs a = {g, "wa_grid_pose_paths", dirs, K, tool, max_turn};
    if (!start_ids || !end_ids || !off || !ids_out || !dir_out || !hops_out || n_pairs < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", a.fn);   // (len_out may be NULL)
    return pose_paths(a, pose_hops(a), start_ids, end_ids, pin_start, pin_end, n_pairs, off, ids_out, dir_out, hops_out, len_out);
}
