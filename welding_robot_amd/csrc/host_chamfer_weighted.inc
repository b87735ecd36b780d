// host_chamfer_weighted.inc -- C ABI: exact shortest paths on the 26-neighbour lattice of free voxels where a move costs its step weight
// plus the penalty of the voxel entered (included by weldacs.hip inside extern "C", behind host_chamfer.inc, whose step check it uses; the
// fourth user of host_geodesic.inc's search driver: this file holds the penalty upload and check, the SearchKind of the two-stage ring and
// the PathSteps of its walk-back).  The calls are stateless: the penalty array is uploaded, checked and packed by every call.

// what a call keeps of its penalty array on the device: the bytes (the walk-back reads them), the five bit planes and P
struct CwPens {
    DevBuf<uint8_t> bytes;
    DevBuf<unsigned long long> planes;
    int32_t P = 0;
};

// uploads and packs the penalties; WA_ERR_ARG for a free voxel whose penalty is above WA_PEN_MAX and for a grid whose largest possible
// distance (M + P) * (n_free - 1) does not fit int32.  Needs g->fbits.  No search has been enqueued when this returns.
static int cw_pens(const wa_grid *g, const WaGeoDims &d, const WaChmStep &cs, const uint8_t *pen, const char *fn, CwPens *cp)
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
    cp->P = 0;
    for (int32_t q = 1; q <= WA_PEN_MAX; q++)
        if (info[1 + q]) cp->P = q;
    if ((int64_t)(cs.M + cp->P) * (g->n_free - 1) > (int64_t)INT32_MAX)
        return fail(ctx, WA_ERR_ARG, "%s: (largest step + largest penalty) * (free voxels - 1) exceeds 2^31 - 1, a distance might not fit int32", fn);
    return WA_OK;
}

// the pull-then-schedule search: `seen` is the arrived bitmap, a source's ring of R = M + P + 1 settled sets is contiguous and zeroed
// whole, level L reads slots (L - step) mod R and writes slots L .. L + P, and a source is alive while one of the last M + P levels had
// an arrival
static SearchKind cw_kind(const wa_grid *g, const WaGeoDims &d, const WaChmStep &cs, const CwPens &cp, const char *fn)
{
    WaCwStep st;
    for (int k = 0; k < 3; k++) st.s[k] = cs.s[k];
    st.M = cs.M; st.P = cp.P;
    const int32_t R = st.M + st.P + 1;
    SearchKind k;
    k.fn = fn;
    k.frontiers = R; k.zeroed = R; k.window = st.M + st.P;
    k.words = d.nw; k.ints = d.n;
    // the largest distance is at most (M + P) * (n_free - 1) <= 2^31 - 1 (cw_pens); R more launches see the ring empty
    k.first = 1; k.bound = std::min<int64_t>((int64_t)(st.M + st.P) * (g->n_free - 1) + R + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    hipStream_t stream = g->ctx->stream;
    const unsigned long long *planes = cp.planes;
    k.seed = [=](const SearchChunk &c, int32_t ns) {
        k_cw_seed<<<(unsigned)((ns + 255) / 256), 256, 0, stream>>>(c.src, ns, d, R, c.seen, c.fronts, c.field, c.last, c.stop);
    };
    k.level = [=](const SearchChunk &c, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
        k_cw_level<<<grid, 256, 0, stream>>>(g->fbits, planes, d, (int32_t)level, (int32_t)(level % R), st, c.seen, c.fronts, c.field, c.last, c.stop, d_tgt, n_tgt, c.mat);
    };
    return k;
}

int wa_grid_chamfer_weighted_fields(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *src_ids, int32_t n_src, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!step || !pen || !src_ids || !dist_out || n_src < 0) return fail(g->ctx, WA_ERR_ARG, "wa_grid_chamfer_weighted_fields: bad argument");
    WaChmStep cs;
    int rc = chm_steps(g, step, "wa_grid_chamfer_weighted_fields", &cs);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, "wa_grid_chamfer_weighted_fields", &src_ids, 1, n_src, &d);
    if (rc || n_src == 0) return rc;
    CwPens cp;
    rc = cw_pens(g, d, cs, pen, "wa_grid_chamfer_weighted_fields", &cp);
    if (rc) return rc;
    return search_rows(g, d, cw_kind(g, d, cs, cp, "wa_grid_chamfer_weighted_fields"), src_ids, n_src, false, dist_out);
}

int wa_grid_chamfer_weighted_matrix(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *point_ids, int32_t n_pts, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!step || !pen || !point_ids || !dist_out || n_pts < 0) return fail(g->ctx, WA_ERR_ARG, "wa_grid_chamfer_weighted_matrix: bad argument");
    WaChmStep cs;
    int rc = chm_steps(g, step, "wa_grid_chamfer_weighted_matrix", &cs);
    if (rc) return rc;
    WaGeoDims d;
    rc = search_begin(g, "wa_grid_chamfer_weighted_matrix", &point_ids, 1, n_pts, &d);
    if (rc || n_pts == 0) return rc;
    CwPens cp;
    rc = cw_pens(g, d, cs, pen, "wa_grid_chamfer_weighted_matrix", &cp);
    if (rc) return rc;
    return search_rows(g, d, cw_kind(g, d, cs, cp, "wa_grid_chamfer_weighted_matrix"), point_ids, n_pts, true, dist_out);
}

int wa_grid_chamfer_weighted_paths(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *start_ids, const int64_t *end_ids,
                                   int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!step || !pen || !start_ids || !end_ids || !off || !ids_out || !dist_out || !len_out || n_pairs < 0)
        return fail(ctx, WA_ERR_ARG, "wa_grid_chamfer_weighted_paths: bad argument");
    WaChmStep cs;
    int rc = chm_steps(g, step, "wa_grid_chamfer_weighted_paths", &cs);
    if (rc) return rc;
    WaGeoDims d;
    rc = paths_begin(g, "wa_grid_chamfer_weighted_paths", start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    CwPens cp;
    rc = cw_pens(g, d, cs, pen, "wa_grid_chamfer_weighted_paths", &cp);
    if (rc) return rc;
    // both passes are k_cw_walkback; the writing pass reads the counts the counting pass left on the device
    DevBuf<int32_t> d_dist, d_len;
    PathSteps steps;
    steps.need = "len_out";
    steps.count = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *dist, int32_t *len) {
        hipError_t e = d_dist.alloc((size_t)np);
        e = e ? e : d_len.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_cw_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, g->occ, cp.bytes, d, cs, d_slot, d_end, nullptr, np, d_dist, d_len, nullptr);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(dist, d_dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(len, d_len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        return e ? e : hipStreamSynchronize(ctx->stream);
    };
    steps.write = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_cw_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, g->occ, cp.bytes, d, cs, d_slot, d_end, d_dst, np, d_dist, d_len, d_out);
        return hipGetLastError();
    };
    return search_paths(g, d, cw_kind(g, d, cs, cp, "wa_grid_chamfer_weighted_paths"), steps, start_ids, end_ids, n_pairs, off, ids_out, dist_out, len_out);
}
