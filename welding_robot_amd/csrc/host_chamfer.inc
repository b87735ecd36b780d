// host_chamfer.inc -- C ABI: exact shortest paths on the 26-neighbour lattice of free voxels with integer step weights, and the same where a
// move also pays the penalty of the voxel entered (included by weldacs.hip inside extern "C", behind host_weighted.inc; the third user of
// host_geodesic.inc's search driver: this file holds the step check, the penalty upload and check, the SearchKind of the pull-form ring
// and the walk-back's launch).  The calls are stateless: the penalty array is uploaded, checked and packed by every weighted call.
// The six exports are two bodies: chm_rows_call (fields, matrix) and chm_paths_call, which take the exported name and `weighted`.

// the three step weights, each in 1 .. WA_STEP_MAX, and max(step) * (n_free - 1) within int32; WA_ERR_ARG otherwise, before anything else is looked at
static int chm_steps(const wa_grid *g, const int32_t step[3], const char *fn, WaChmStep *st)
{
    wa_ctx *ctx = g->ctx;
    st->M = 0; st->P = 0;
    for (int k = 0; k < 3; k++) {
        if (step[k] < 1 || step[k] > WA_STEP_MAX) return fail(ctx, WA_ERR_ARG, "%s: a step weight outside 1 .. WA_STEP_MAX", fn);
        st->s[k] = step[k];
        st->M = std::max(st->M, step[k]);
    }
    if ((int64_t)st->M * (std::max<int64_t>(g->n_free, 1) - 1) > (int64_t)INT32_MAX)
        return fail(ctx, WA_ERR_ARG, "%s: (largest step) * (free voxels - 1) exceeds 2^31 - 1, a distance might not fit int32", fn);
    return WA_OK;
}

// what a weighted call keeps of its penalty array on the device: the bytes (the walk-back reads them) and the five bit planes
struct CwPens {
    DevBuf<uint8_t> bytes;
    DevBuf<unsigned long long> planes;
};

// uploads and packs the penalties and sets st->P; WA_ERR_ARG for a free voxel whose penalty is above WA_PEN_MAX and for a grid whose
// largest possible distance (M + P) * (n_free - 1) does not fit int32.  Needs g->fbits.  No search has been enqueued when this returns.
static int cw_pens(const wa_grid *g, const WaGeoDims &d, const uint8_t *pen, const char *fn, WaChmStep *st, CwPens *cp)
{
    wa_ctx *ctx = g->ctx;
    DevBuf<int32_t> d_info;
    int32_t info[WA_PEN_MAX + 2];
    hipError_t e = cp->bytes.alloc((size_t)d.n);
    e = e ? e : cp->planes.alloc((size_t)(WA_PEN_PLANES * d.nw));
    e = e ? e : d_info.alloc((size_t)(WA_PEN_MAX + 2));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_ALLOC, "%s: the penalty array does not fit the device", fn); }
    e = hipMemcpyAsync(cp->bytes, pen, (size_t)d.n, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(d_info, 0, sizeof info, ctx->stream);
    if (e == hipSuccess) {
        k_cw_planes<<<(unsigned)((d.nw + 3) / 4), 256, 0, ctx->stream>>>(g->occ, cp->bytes, d, cp->planes, d_info);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: packing the penalties: %s", fn, hipGetErrorString(e));
    if (info[0]) return fail(ctx, WA_ERR_ARG, "%s: a free voxel's penalty is above WA_PEN_MAX", fn);
    st->P = 0;
    for (int32_t q = 1; q <= WA_PEN_MAX; q++)
        if (info[1 + q]) st->P = q;
    if ((int64_t)(st->M + st->P) * (g->n_free - 1) > (int64_t)INT32_MAX)
        return fail(ctx, WA_ERR_ARG, "%s: (largest step + largest penalty) * (free voxels - 1) exceeds 2^31 - 1, a distance might not fit int32", fn);
    return WA_OK;
}

// the pull-form search: `seen` is the done / arrived bitmap, a source's ring of R = M + P + 1 settled sets is contiguous and zeroed
// whole, level L reads slots (L - step) mod R and writes slots L .. L + P, and a source is alive while one of the last M + P levels had
// an arrival.  planes == NULL: no penalties (st.P is 0), the kernel without the penalty stage.
static SearchKind chm_kind(const wa_grid *g, const WaGeoDims &d, const WaChmStep &st, const unsigned long long *planes, const char *fn)
{
    const int32_t R = st.M + st.P + 1;
    SearchKind k;
    k.fn = fn;
    k.frontiers = R; k.zeroed = R; k.window = st.M + st.P;
    k.words = d.nw; k.ints = d.n;
    // the largest distance is at most (M + P) * (n_free - 1) <= 2^31 - 1 (chm_steps, cw_pens); R more launches see the ring empty
    k.first = 1; k.bound = std::min<int64_t>((int64_t)(st.M + st.P) * (g->n_free - 1) + R + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    hipStream_t stream = g->ctx->stream;
    k.seed = [=](const SearchChunk &c, int32_t ns) {
        k_geo_ring_seed<<<(unsigned)((ns + 255) / 256), 256, 0, stream>>>(c.src, ns, d, R, c.seen, c.fronts, c.field, c.last, c.stop);
    };
    k.level = [=](const SearchChunk &c, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
        const auto kernel = planes ? k_chm_ring_level<true> : k_chm_ring_level<false>;
        kernel<<<grid, 256, 0, stream>>>(g->fbits, planes, d, (int32_t)level, (int32_t)(level % R), st, c.seen, c.fronts, c.field, c.last, c.stop, d_tgt, n_tgt, c.mat);
    };
    return k;
}

// _fields (points == false) and _matrix of both families behind their names.  The order of the checks is the contract: arguments, steps,
// ids, nothing more for a count of 0, then the penalties.
static int chm_rows_call(const char *fn, const wa_grid *g, const int32_t step[3], bool weighted, const uint8_t *pen, const int64_t *ids, int32_t n,
                         bool points, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!step || (weighted && !pen) || !ids || !dist_out || n < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", fn);
    WaChmStep st;
    int rc = chm_steps(g, step, fn, &st);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, fn, &ids, 1, n, &d);
    if (rc || n == 0) return rc;
    CwPens cp;
    rc = weighted ? cw_pens(g, d, pen, fn, &st, &cp) : WA_OK;
    if (rc) return rc;
    return search_rows(g, d, chm_kind(g, d, st, cp.planes, fn), ids, n, points, dist_out);
}

// _paths of both families, the same order of checks; both passes are k_chm_walkback (walkback_steps)
static int chm_paths_call(const char *fn, const wa_grid *g, const int32_t step[3], bool weighted, const uint8_t *pen, const int64_t *start_ids,
                          const int64_t *end_ids, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!step || (weighted && !pen) || !start_ids || !end_ids || !off || !ids_out || !dist_out || !len_out || n_pairs < 0)
        return fail(ctx, WA_ERR_ARG, "%s: bad argument", fn);
    WaChmStep st;
    int rc = chm_steps(g, step, fn, &st);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, fn, start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    CwPens cp;
    rc = weighted ? cw_pens(g, d, pen, fn, &st, &cp) : WA_OK;
    if (rc) return rc;
    WalkbackCounts counts;
    const PathSteps steps = walkback_steps(ctx, &counts, [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst,
                                                             int32_t np, int32_t *d_dist, int32_t *d_len, long long *d_out) {
        const auto kernel = weighted ? k_chm_walkback<true> : k_chm_walkback<false>;
        kernel<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, g->occ, cp.bytes, d, st, d_slot, d_end, d_dst, np, d_dist, d_len, d_out);
    });
    return search_paths(g, d, chm_kind(g, d, st, cp.planes, fn), steps, start_ids, end_ids, n_pairs, off, ids_out, dist_out, len_out);
}

int wa_grid_chamfer_fields(const wa_grid *g, const int32_t step[3], const int64_t *src_ids, int32_t n_src, int32_t *dist_out)
{
    return chm_rows_call("wa_grid_chamfer_fields", g, step, false, nullptr, src_ids, n_src, false, dist_out);
}

int wa_grid_chamfer_matrix(const wa_grid *g, const int32_t step[3], const int64_t *point_ids, int32_t n_pts, int32_t *dist_out)
{
    return chm_rows_call("wa_grid_chamfer_matrix", g, step, false, nullptr, point_ids, n_pts, true, dist_out);
}

int wa_grid_chamfer_paths(const wa_grid *g, const int32_t step[3], const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                          const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    return chm_paths_call("wa_grid_chamfer_paths", g, step, false, nullptr, start_ids, end_ids, n_pairs, off, ids_out, dist_out, len_out);
}

int wa_grid_chamfer_weighted_fields(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *src_ids, int32_t n_src, int32_t *dist_out)
{
    return chm_rows_call("wa_grid_chamfer_weighted_fields", g, step, true, pen, src_ids, n_src, false, dist_out);
}

int wa_grid_chamfer_weighted_matrix(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *point_ids, int32_t n_pts, int32_t *dist_out)
{
    return chm_rows_call("wa_grid_chamfer_weighted_matrix", g, step, true, pen, point_ids, n_pts, true, dist_out);
}

int wa_grid_chamfer_weighted_paths(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *start_ids, const int64_t *end_ids,
                                   int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    return chm_paths_call("wa_grid_chamfer_weighted_paths", g, step, true, pen, start_ids, end_ids, n_pairs, off, ids_out, dist_out, len_out);
}
