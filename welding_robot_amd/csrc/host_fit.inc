// host_fit.inc -- C ABI: the trajectory fit that refines its control polygon until the sampled curve clears the grid
// (included by weldacs.hip inside extern "C").  Everything between the arguments and the results stays on the device, on the
// context's stream; per round the host reads one WaFitRec (the next fit's size, the hit count, whether a level changed).
// The loop itself is fit_run, which takes the round's segment test as a callable: wa_grid_pose_fit_trajectory (host_pose_fit.inc) runs it too.
struct FitBuffers {
    DevBuf<int32_t> level, owner, d2;
    DevBuf<uint8_t> mark, hit;
    DevBuf<long long> off, bsum, ids;
    DevBuf<WaFitRec> rec;
    OwnedHandle<wa_traj> samples;
    OwnedHandle<wa_bspline> b;
    long long cap_cps = 0;
};

// pieces at the current levels, scanned: off[0 .. n_legs], rec->total
static hipError_t fit_pieces(wa_ctx *ctx, const wa_traj *poly, FitBuffers &B, double spacing)
{
    const long long n_legs = poly->n - 1;
    const unsigned blocks = (unsigned)((n_legs + 255) / 256);
    k_fit_pieces<<<blocks, 256, 0, ctx->stream>>>(poly->xyz, n_legs, B.level, spacing, B.off, B.bsum, B.rec);
    k_fit_scan_sums<<<1, 256, 0, ctx->stream>>>(B.bsum, (long long)blocks, B.rec);
    k_fit_scan_add<<<(unsigned)((n_legs + 1 + 255) / 256), 256, 0, ctx->stream>>>(B.off, n_legs, B.bsum, B.rec);
    return hipGetLastError();
}

// room for a spline of n_cps control points in B.b (kept from round to round, grown by half when a round needs more)
static hipError_t fit_spline_room(wa_ctx *ctx, FitBuffers &B, int32_t degree, long long n_cps)
{
    if (!B.b) {
        B.b.reset(new wa_bspline());
        B.b->ctx = ctx;
        B.b->S.knots = nullptr; B.b->S.cps = nullptr; B.b->S.uninit = 0.0f;
        B.b->d_ends = nullptr;
        B.b->set = false;
    }
    WaSpline &S = B.b->S;
    S.dim = 3; S.degree = degree; S.ci = degree - 1; S.cf = degree - 1;
    S.n_cps = n_cps;
    S.n_middle = n_cps - 2 * degree;              // BSplineBasic.h:40
    S.n_knots = n_cps + degree + 1;               // :38-39
    if (n_cps <= B.cap_cps) return hipSuccess;
    dev_free(S.knots); dev_free(S.cps);   // (the spline's own: it grows by half)
    S.knots = nullptr; S.cps = nullptr;
    B.cap_cps = 0;
    const long long cap = std::min(n_cps + n_cps / 2, (long long)WA_FIT_MAX_CPS);
    hipError_t e = dalloc(&S.knots, (size_t)(cap + degree + 1));
    e = e ? e : dalloc(&S.cps, (size_t)cap * 3);
    e = e ? e : B.owner.alloc((size_t)cap);
    if (e == hipSuccess && !B.b->d_ends) e = dalloc(&B.b->d_ends, (size_t)(2 * degree) * 3);
    if (e == hipSuccess) B.cap_cps = cap;
    return e;
}

// the segment test of a round: enqueues on the context's stream what fills B.hit (one byte per segment, non-zero: refine around it) and
// the record's acc[1] (the first such segment) and acc[2] (their number) from the round's sample voxels B.ids
using FitSegTest = std::function<hipError_t(const FitBuffers &B, const WaSpline &S, float dt)>;

// the arguments every fit shares, behind the caller's check of g: 0 or WA_ERR_ARG
static int fit_check(wa_ctx *ctx, const char *fn, const wa_traj *poly, const void *sum, const void *spline_out, int32_t degree, float spacing,
                     int32_t max_level, int64_t n_samples)
{
    if (!poly || !sum || !spline_out) return fail(ctx, WA_ERR_ARG, "%s: NULL polyline, summary or spline output", fn);
    if (poly->ctx != ctx) return fail(ctx, WA_ERR_ARG, "%s: polyline and grid belong to different contexts", fn);
    if (poly->n < 2) return fail(ctx, WA_ERR_ARG, "%s: a polyline needs at least 2 points", fn);
    if (degree != 2 && degree != 3) return fail(ctx, WA_ERR_ARG, "%s: degree must be 2 or 3", fn);
    if (!(spacing > 0.0f) || !isfinite(spacing)) return fail(ctx, WA_ERR_ARG, "%s: spacing must be finite and > 0", fn);
    if (max_level < 0 || max_level > WA_FIT_MAX_LEVEL) return fail(ctx, WA_ERR_ARG, "%s: max_level must be 0..8", fn);
    if (n_samples < 2 || n_samples > ((int64_t)1 << 33)) return fail(ctx, WA_ERR_ARG, "%s: n_samples must be 2..2^33", fn);
    if (poly->n - 1 > WA_FIT_MAX_CPS) return fail(ctx, WA_ERR_ARG, "%s: more than 2^24 control points", fn);
    return WA_OK;
}

// The loop both fits run, behind fit_check: control polygon -> fit -> sample -> `test` -> blame -> refine, until the test marks no
// segment or nothing can be refined.  Leaves the last round's spline and samples in B, its levels in *lv, its record in *rec_out and the
// summary's fields in *s (n_hit_first and final's segment terms are whatever `test` counted).  Nothing of the caller's is written.
static int fit_run(const wa_grid *g, const char *fn, const wa_traj *poly, int32_t degree, float spacing, int32_t max_level, int64_t n_samples,
                   const FitSegTest &test, FitBuffers &B, wa_fit_summary *s_out, WaFitRec *rec_out, std::vector<int32_t> *lv)
{
    wa_ctx *ctx = g->ctx;
    const long long n_legs = poly->n - 1;
    WaField F;
    int rc = grid_field(g, &F);
    if (rc) return rc;

    const long long n_seg = n_samples - 1;
    hipError_t e = B.level.alloc((size_t)n_legs);
    e = e ? e : B.mark.alloc((size_t)n_legs);
    e = e ? e : B.off.alloc((size_t)n_legs + 1);
    e = e ? e : B.bsum.alloc((size_t)((n_legs + 255) / 256));
    e = e ? e : B.rec.alloc(1);
    e = e ? e : B.ids.alloc((size_t)n_samples);
    e = e ? e : B.d2.alloc((size_t)n_samples);
    e = e ? e : B.hit.alloc((size_t)n_seg);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", fn);
    wa_traj *samples = nullptr;
    rc = traj_alloc(ctx, n_samples, &samples);
    if (rc) return rc;
    B.samples.reset(samples);
    e = hipMemsetAsync(B.level, 0, sizeof(int32_t) * n_legs, ctx->stream);
    e = e ? e : hipMemsetAsync(B.mark, 0, (size_t)n_legs, ctx->stream);
    e = e ? e : hipMemsetAsync(B.rec, 0, sizeof(WaFitRec), ctx->stream);
    e = e ? e : fit_pieces(ctx, poly, B, (double)spacing);
    WaFitRec rec;
    e = e ? e : hipMemcpyAsync(&rec, B.rec, sizeof rec, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    if (rec.bad) return fail(ctx, WA_ERR_ARG, "%s: a coordinate of the polyline is not finite", fn);

    wa_fit_summary s;
    memset(&s, 0, sizeof s);
    s.n_legs = n_legs;
    for (int32_t round = 0;; round++) {
        // the control polygon has rec.total + 1 points: two end positions and rec.total - 1 middle points
        const long long n_cps = rec.total - 1 + 2 * degree;
        if (rec.total > WA_FIT_MAX_CPS || n_cps > WA_FIT_MAX_CPS) return fail(ctx, WA_ERR_ARG, "%s: more than 2^24 control points", fn);
        e = fit_spline_room(ctx, B, degree, n_cps);
        if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: spline buffers", fn);
        const WaSpline &S = B.b->S;
        const float fin_time = (float)(S.n_knots - 2 * degree - 1);   // the number of knot spans: the chain's step is exactly 1.0f
        const float dt = fin_time / (float)(n_samples - 1);
        const int32_t last = round == WA_FIT_MAX_ROUNDS - 1;
        k_fit_emit<<<(unsigned)((rec.total + 1 + 255) / 256), 256, 0, ctx->stream>>>(poly->xyz, n_legs, B.off, S, B.owner);
        k_fit_knots<<<(unsigned)((S.n_knots + 255) / 256), 256, 0, ctx->stream>>>(S, fin_time);
        k_fit_ends<<<1, 64, 0, ctx->stream>>>(poly->xyz, n_legs, S, B.b->d_ends, fin_time, B.owner, B.rec);
        e = hipGetLastError();
        e = e ? e : bspline_launch(B.b.get(), nullptr, 0.0f, dt, n_samples, 0, B.samples->xyz, nullptr);
        if (e == hipSuccess) {
            k_clr_samples<<<(unsigned)((n_samples + 255) / 256), 256, 0, ctx->stream>>>(B.samples->xyz, n_samples, F, B.ids, B.d2, B.rec.p->acc);
            e = hipGetLastError();
        }
        e = e ? e : test(B, S, dt);
        if (e == hipSuccess) {
            if (degree == 2) k_fit_blame<2><<<(unsigned)((n_seg + 255) / 256), 256, 0, ctx->stream>>>(S, B.hit, n_seg, dt, B.owner, B.mark);
            else k_fit_blame<3><<<(unsigned)((n_seg + 255) / 256), 256, 0, ctx->stream>>>(S, B.hit, n_seg, dt, B.owner, B.mark);
            k_fit_bump<<<(unsigned)((n_legs + 255) / 256), 256, 0, ctx->stream>>>(B.level, B.mark, n_legs, max_level, last ? 0 : 1, B.rec);
            e = hipGetLastError();
        }
        e = e ? e : fit_pieces(ctx, poly, B, (double)spacing);   // (the next round's, should there be one)
        e = e ? e : hipMemcpyAsync(&rec, B.rec, sizeof rec, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
        const int64_t n_hit = (int64_t)rec.acc[2];
        if (round == 0) s.n_hit_first = n_hit;
        s.rounds = round + 1;
        if (n_hit == 0 || rec.changed == 0 || last) break;
    }
    s.n_legs_at_cap = rec.at_cap;
    s.n_cps = B.b->S.n_cps;
    clr_summary_from(rec.acc, &s.final);
    lv->resize((size_t)n_legs);
    e = hipMemcpy(lv->data(), B.level, sizeof(int32_t) * n_legs, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    for (int32_t v : *lv) s.max_level_used = std::max(s.max_level_used, v);
    *s_out = s;
    *rec_out = rec;
    return WA_OK;
}

int wa_grid_fit_trajectory(const wa_grid *g, const wa_traj *poly, int32_t degree, float spacing, int32_t max_level, int64_t n_samples,
                           int32_t *leg_level_out, wa_bspline **spline_out, wa_traj **samples_out, wa_fit_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_fit_trajectory";
    int rc = fit_check(ctx, fn, poly, sum, spline_out, degree, spacing, max_level, n_samples);
    if (rc) return rc;
    FitBuffers B;
    wa_fit_summary s;
    WaFitRec rec;
    std::vector<int32_t> lv;
    const unsigned seg_blocks = (unsigned)((n_samples - 1 + 255) / 256);
    rc = fit_run(g, fn, poly, degree, spacing, max_level, n_samples, [&](const FitBuffers &R, const WaSpline &, float) {
        k_clr_segments<<<seg_blocks, 256, 0, ctx->stream>>>(R.ids, n_samples, g->d, g->occ, R.hit, R.rec.p->acc);
        return hipGetLastError();
    }, B, &s, &rec, &lv);
    if (rc) return rc;
    if (leg_level_out) memcpy(leg_level_out, lv.data(), sizeof(int32_t) * lv.size());
    B.b->set = true;
    B.b->h_valid = false;
    *spline_out = B.b.release();
    if (samples_out) *samples_out = B.samples.release();
    *sum = s;
    return WA_OK;
}
