// host_weighted.inc -- C ABI: clearance costs, and exact shortest paths with per-voxel entry costs on the 6-neighbour lattice of free voxels
// (included by weldacs.hip inside extern "C", behind host_geodesic.inc, whose search driver it runs on: this file holds what is weighted about the
// search, SearchKind and PathSteps say where it plugs in).  The calls are stateless: the cost array is uploaded, checked and packed by every call.

int wa_grid_clearance_costs(const wa_grid *g, const int32_t *thr2, int32_t n_thr, uint8_t *cost_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!thr2 || !cost_out || n_thr < 0 || n_thr > WA_COST_MAX - 1) return fail(ctx, WA_ERR_ARG, "wa_grid_clearance_costs: bad argument");
    WaThr2 t;
    t.n = n_thr;
    for (int32_t k = 0; k < WA_COST_MAX - 1; k++) t.v[k] = 0;
    for (int32_t k = 0; k < n_thr; k++) {
        if (thr2[k] < 0 || thr2[k] >= WA_D2_NONE) return fail(ctx, WA_ERR_ARG, "wa_grid_clearance_costs: a threshold outside 0 .. WA_D2_NONE - 1");
        t.v[k] = thr2[k];
    }
    int rc = grid_build_d2(g);
    if (rc) return rc;
    const int64_t n = g->d.n;
    DevBuf<uint8_t> d_cost;
    if (d_cost.alloc((size_t)n) != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_grid_clearance_costs: the cost array");
    k_wgt_clearance_costs<<<(unsigned)((n + 1023) / 1024), 256, 0, ctx->stream>>>(g->occ, g->d2, n, t, d_cost);
    hipError_t e = hipGetLastError();
    e = e ? e : hipMemcpyAsync(cost_out, d_cost, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_clearance_costs: %s", hipGetErrorString(e));
    return WA_OK;
}

// what a call keeps of its cost array on the device: the bytes (the walk-back reads them), the three bit planes and W
struct WgtCosts {
    DevBuf<uint8_t> bytes;
    DevBuf<unsigned long long> planes;
    int32_t W = 0;
};

// uploads and packs the costs; WA_ERR_ARG for a free voxel whose cost is outside 1 .. WA_COST_MAX and for a grid whose largest
// possible distance W * (n_free - 1) does not fit int32.  Needs g->fbits.
static int wgt_costs(const wa_grid *g, const WaGeoDims &d, const uint8_t *cost, const char *fn, WgtCosts *wc)
{
    wa_ctx *ctx = g->ctx;
    DevBuf<int32_t> d_info;
    int32_t info[WA_COST_MAX + 1];
    hipError_t e = wc->bytes.alloc((size_t)d.n);
    e = e ? e : wc->planes.alloc((size_t)(3 * d.nw));
    e = e ? e : d_info.alloc((size_t)(WA_COST_MAX + 1));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_ALLOC, "%s: the cost array does not fit the device", fn); }
    e = hipMemcpyAsync(wc->bytes, cost, (size_t)d.n, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(d_info, 0, sizeof info, ctx->stream);
    if (e == hipSuccess) {
        k_wgt_planes<<<(unsigned)((d.nw + 3) / 4), 256, 0, ctx->stream>>>(g->occ, wc->bytes, d, wc->planes, d_info);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: packing the costs: %s", fn, hipGetErrorString(e));
    if (info[0]) return fail(ctx, WA_ERR_ARG, "%s: a free voxel's cost is outside 1 .. WA_COST_MAX", fn);
    wc->W = 1;   // (a grid without a free voxel cannot get here: the ids are checked first)
    for (int32_t c = 1; c <= WA_COST_MAX; c++)
        if (info[c]) wc->W = c;
    if ((int64_t)wc->W * (g->n_free - 1) > (int64_t)INT32_MAX)
        return fail(ctx, WA_ERR_ARG, "%s: (largest cost) * (free voxels - 1) exceeds 2^31 - 1, a distance might not fit int32", fn);
    return WA_OK;
}

// the search with entry costs: `seen` is the touched bitmap, a source's ring of R = W + 1 frontiers is contiguous and zeroed whole, level
// L works on slot L mod R, and a source is alive while one of the last R launches saw a frontier or touched a voxel
static SearchKind wgt_kind(const wa_grid *g, const WaGeoDims &d, const WgtCosts &wc, const char *fn)
{
    const int32_t W = wc.W, R = W + 1;
    SearchKind k;
    k.fn = fn;
    k.frontiers = R; k.zeroed = R; k.window = R;
    k.words = d.nw; k.ints = d.n;
    // the largest distance is at most W * (n_free - 1) <= 2^31 - 1 (wgt_costs); R more launches see the ring empty
    k.first = 0; k.bound = std::min<int64_t>((int64_t)W * (g->n_free - 1) + R + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    hipStream_t st = g->ctx->stream;
    const unsigned long long *planes = wc.planes;
    k.seed = [=](const SearchChunk &c, int32_t ns) {
        k_geo_ring_seed<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(c.src, ns, d, R, c.seen, c.fronts, nullptr, c.last, c.stop);   // (level 0 writes the field's 0)
    };
    k.level = [=](const SearchChunk &c, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
        k_wgt_level<<<grid, 256, 0, st>>>(g->fbits, planes, d, (int32_t)level, (int32_t)(level % R), W, c.seen, c.fronts, c.field, c.last, c.stop, d_tgt, n_tgt, c.mat);
    };
    return k;
}

// wa_grid_weighted_fields (points == false) and _matrix behind their names
static int wgt_rows_call(const char *fn, const wa_grid *g, const uint8_t *cost, const int64_t *ids, int32_t n, bool points, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!cost || !ids || !dist_out || n < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", fn);
    WaGeoDims d;
    int rc = search_begin(g, fn, &ids, 1, n, &d);
    if (rc || n == 0) return rc;
    WgtCosts wc;
    rc = wgt_costs(g, d, cost, fn, &wc);
    if (rc) return rc;
    return search_rows(g, d, wgt_kind(g, d, wc, fn), ids, n, points, dist_out);
}

int wa_grid_weighted_fields(const wa_grid *g, const uint8_t *cost, const int64_t *src_ids, int32_t n_src, int32_t *dist_out)
{
    return wgt_rows_call("wa_grid_weighted_fields", g, cost, src_ids, n_src, false, dist_out);
}

int wa_grid_weighted_matrix(const wa_grid *g, const uint8_t *cost, const int64_t *point_ids, int32_t n_pts, int32_t *dist_out)
{
    return wgt_rows_call("wa_grid_weighted_matrix", g, cost, point_ids, n_pts, true, dist_out);
}

int wa_grid_weighted_paths(const wa_grid *g, const uint8_t *cost, const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                           const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!cost || !start_ids || !end_ids || !off || !ids_out || !dist_out || !len_out || n_pairs < 0)
        return fail(ctx, WA_ERR_ARG, "wa_grid_weighted_paths: bad argument");
    WaGeoDims d;
    int rc = paths_begin(g, "wa_grid_weighted_paths", start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    WgtCosts wc;
    rc = wgt_costs(g, d, cost, "wa_grid_weighted_paths", &wc);
    if (rc) return rc;
    WalkbackCounts counts;
    const PathSteps steps = walkback_steps(ctx, &counts, [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst,
                                                             int32_t np, int32_t *d_dist, int32_t *d_len, long long *d_out) {
        k_wgt_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, wc.bytes, d, d_slot, d_end, d_dst, np, d_dist, d_len, d_out);
    });
    return search_paths(g, d, wgt_kind(g, d, wc, "wa_grid_weighted_paths"), steps, start_ids, end_ids, n_pairs, off, ids_out, dist_out, len_out);
}
