// host_chamfer.inc -- C ABI: exact shortest paths on the 26-neighbour lattice of free voxels with integer step weights (included by weldacs.hip
// inside extern "C", behind host_weighted.inc; the third user of host_geodesic.inc's search driver: this file holds the step check, the
// SearchKind of the pull-form ring and the PathSteps of the 26-offset walk-back).  The calls are stateless.

// the three step weights, each in 1 .. WA_STEP_MAX, and max(step) * (n_free - 1) within int32; WA_ERR_ARG otherwise, before anything else is looked at
static int chm_steps(const wa_grid *g, const int32_t step[3], const char *fn, WaChmStep *st)
{
    wa_ctx *ctx = g->ctx;
    st->M = 0;
    for (int k = 0; k < 3; k++) {
        if (step[k] < 1 || step[k] > WA_STEP_MAX) return fail(ctx, WA_ERR_ARG, "%s: a step weight outside 1 .. WA_STEP_MAX", fn);
        st->s[k] = step[k];
        st->M = std::max(st->M, step[k]);
    }
    if ((int64_t)st->M * (std::max<int64_t>(g->n_free, 1) - 1) > (int64_t)INT32_MAX)
        return fail(ctx, WA_ERR_ARG, "%s: (largest step) * (free voxels - 1) exceeds 2^31 - 1, a distance might not fit int32", fn);
    return WA_OK;
}

// the pull-form search: `seen` is the done bitmap, a source's ring of R = M + 1 settled sets is contiguous and zeroed whole, level L
// writes slot L mod R, and a source is alive while one of the last M levels settled a voxel
static SearchKind chm_kind(const wa_grid *g, const WaGeoDims &d, const WaChmStep &cs, const char *fn)
{
    const int32_t R = cs.M + 1;
    SearchKind k;
    k.fn = fn;
    k.frontiers = R; k.zeroed = R; k.window = cs.M;
    k.words = d.nw; k.ints = d.n;
    // the largest distance is at most M * (n_free - 1) <= 2^31 - 1 (chm_steps); R more launches see the ring empty
    k.first = 1; k.bound = std::min<int64_t>((int64_t)cs.M * (g->n_free - 1) + R + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    hipStream_t st = g->ctx->stream;
    k.seed = [=](const SearchChunk &c, int32_t ns) {
        k_chm_seed<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(c.src, ns, d, R, c.seen, c.fronts, c.field, c.last, c.stop);
    };
    k.level = [=](const SearchChunk &c, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
        k_chm_level<<<grid, 256, 0, st>>>(g->fbits, d, (int32_t)level, (int32_t)(level % R), cs, c.seen, c.fronts, c.field, c.last, c.stop, d_tgt, n_tgt, c.mat);
    };
    return k;
}

int wa_grid_chamfer_fields(const wa_grid *g, const int32_t step[3], const int64_t *src_ids, int32_t n_src, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!step || !src_ids || !dist_out || n_src < 0) return fail(g->ctx, WA_ERR_ARG, "wa_grid_chamfer_fields: bad argument");
    WaChmStep cs;
    int rc = chm_steps(g, step, "wa_grid_chamfer_fields", &cs);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, "wa_grid_chamfer_fields", &src_ids, 1, n_src, &d);
    if (rc || n_src == 0) return rc;
    return search_rows(g, d, chm_kind(g, d, cs, "wa_grid_chamfer_fields"), src_ids, n_src, false, dist_out);
}

int wa_grid_chamfer_matrix(const wa_grid *g, const int32_t step[3], const int64_t *point_ids, int32_t n_pts, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!step || !point_ids || !dist_out || n_pts < 0) return fail(g->ctx, WA_ERR_ARG, "wa_grid_chamfer_matrix: bad argument");
    WaChmStep cs;
    int rc = chm_steps(g, step, "wa_grid_chamfer_matrix", &cs);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, "wa_grid_chamfer_matrix", &point_ids, 1, n_pts, &d);
    if (rc || n_pts == 0) return rc;
    return search_rows(g, d, chm_kind(g, d, cs, "wa_grid_chamfer_matrix"), point_ids, n_pts, true, dist_out);
}

int wa_grid_chamfer_paths(const wa_grid *g, const int32_t step[3], const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                          const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!step || !start_ids || !end_ids || !off || !ids_out || !dist_out || !len_out || n_pairs < 0)
        return fail(ctx, WA_ERR_ARG, "wa_grid_chamfer_paths: bad argument");
    WaChmStep cs;
    int rc = chm_steps(g, step, "wa_grid_chamfer_paths", &cs);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, "wa_grid_chamfer_paths", start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    // both passes are k_chm_walkback; the writing pass reads the counts the counting pass left on the device
    DevBuf<int32_t> d_dist, d_len;
    PathSteps steps;
    steps.need = "len_out";
    steps.count = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *dist, int32_t *len) {
        hipError_t e = d_dist.alloc((size_t)np);
        e = e ? e : d_len.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_chm_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, g->occ, d, cs, d_slot, d_end, nullptr, np, d_dist, d_len, nullptr);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(dist, d_dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(len, d_len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        return e ? e : hipStreamSynchronize(ctx->stream);
    };
    steps.write = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_chm_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, g->occ, d, cs, d_slot, d_end, d_dst, np, d_dist, d_len, d_out);
        return hipGetLastError();
    };
    return search_paths(g, d, chm_kind(g, d, cs, "wa_grid_chamfer_paths"), steps, start_ids, end_ids, n_pairs, off, ids_out, dist_out, len_out);
}
