// host_pose_fit.inc -- C ABI: wa_grid_pose_fit_trajectory, the trajectory fit that refines until a planned direction stays open along
// the sampled curve (included by weldacs.hip inside extern "C", behind host_fit.inc, whose loop fit_run it runs with a segment test of
// its own, and host_reach.inc, whose k_reach launch gives it the masks, once per call, before round 1).  Stateless like the pose calls:
// the masks are recomputed by every call.  Per round the host reads the fit's one WaFitRec; the directions, the blocked bytes and the
// last round's counters come back once, behind the loop.
int wa_grid_pose_fit_trajectory(const wa_grid *g, const wa_traj *poly, int32_t degree, float spacing, int32_t max_level, int64_t n_samples,
                                const float *dirs, int32_t K, const wa_tool_beads *tool, const int32_t *leg_hold, int32_t *leg_level_out,
                                wa_bspline **spline_out, wa_traj **samples_out, int32_t *seg_dir_out, uint8_t *blocked_out,
                                wa_pose_fit_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    const char *fn = "wa_grid_pose_fit_trajectory";
    int rc = fit_check(ctx, fn, poly, sum, spline_out, degree, spacing, max_level, n_samples);
    if (rc) return rc;
    std::vector<short4> hq;
    WaReachTool dt_tool;
    rc = reach_check(ctx, fn, dirs, K, tool, &hq, &dt_tool);
    if (rc) return rc;
    if (!leg_hold) return fail(ctx, WA_ERR_ARG, "%s: NULL leg_hold", fn);
    const long long n_legs = poly->n - 1;
    for (long long k = 0; k < n_legs; k++)
        if (leg_hold[k] < -1 || leg_hold[k] >= K) return fail(ctx, WA_ERR_ARG, "%s: a hold outside -1 .. K - 1", fn);

    hipStream_t st = ctx->stream;
    const int64_t n_seg = n_samples - 1;
    const unsigned seg_blocks = (unsigned)((n_seg + 255) / 256);
    ReachBuffers R(ctx);
    rc = reach_enqueue(g, fn, hq, dt_tool, true, R);
    if (rc) { hipStreamSynchronize(st); return rc; }
    DevBuf<int32_t> d_hold, d_dir;
    DevBuf<unsigned long long> d_cnt;   // [0] n_no_candidate of the round, [1] n_dir_changes, [2] max_dir_turn, [3 .. 6] final's acc
    enum { C_NONE = 0, C_CHANGES, C_TURN, C_ACC, C_SIZE = C_ACC + 4 };
    hipError_t e = d_hold.alloc((size_t)n_legs);
    e = e ? e : d_dir.alloc((size_t)n_seg);
    e = e ? e : d_cnt.alloc(C_SIZE);
    if (e != hipSuccess) { hipStreamSynchronize(st); return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", fn); }
    e = hipMemcpyAsync(d_hold, leg_hold, sizeof(int32_t) * n_legs, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { hipStreamSynchronize(st); return fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e)); }

    FitBuffers B;
    wa_fit_summary fs;
    WaFitRec rec;
    std::vector<int32_t> lv;
    rc = fit_run(g, fn, poly, degree, spacing, max_level, n_samples, [&](const FitBuffers &F, const WaSpline &S, float dt) {
        hipError_t t = hipMemsetAsync(d_cnt.p + C_NONE, 0, sizeof(unsigned long long), st);
        if (t != hipSuccess) return t;
        if (degree == 2)
            k_pfit_segments<2><<<seg_blocks, 256, 0, st>>>(F.ids, n_samples, g->d, g->occ, R.mask.p, S, dt, F.owner, d_hold, F.hit, d_dir,
                                                           F.rec.p->acc, d_cnt.p + C_NONE);
        else
            k_pfit_segments<3><<<seg_blocks, 256, 0, st>>>(F.ids, n_samples, g->d, g->occ, R.mask.p, S, dt, F.owner, d_hold, F.hit, d_dir,
                                                           F.rec.p->acc, d_cnt.p + C_NONE);
        return hipGetLastError();
    }, B, &fs, &rec, &lv);
    if (rc) { hipStreamSynchronize(st); return rc; }

    // behind the last round: its samples against the occupancy (final's segment terms), the direction statistics, and everything home
    unsigned long long cnt[C_SIZE];
    memset(cnt, 0, sizeof cnt);
    clr_acc_init(cnt + C_ACC);
    std::vector<int32_t> seg_dir(seg_dir_out ? (size_t)n_seg : 0);
    std::vector<uint8_t> blocked(blocked_out ? (size_t)n_seg : 0);
    e = hipMemcpyAsync(d_cnt.p + C_CHANGES, cnt + C_CHANGES, sizeof(unsigned long long) * (C_SIZE - C_CHANGES), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        k_clr_segments<<<seg_blocks, 256, 0, st>>>(B.ids, n_samples, g->d, g->occ, nullptr, d_cnt.p + C_ACC);
        k_pfit_dir_stats<<<seg_blocks, 256, 0, st>>>(d_dir, n_seg, R.q, d_cnt.p + C_CHANGES);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && seg_dir_out) e = hipMemcpyAsync(seg_dir.data(), d_dir, sizeof(int32_t) * n_seg, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && blocked_out) e = hipMemcpyAsync(blocked.data(), B.hit, (size_t)n_seg, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    e = e ? e : es;
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));

    wa_pose_fit_summary s;
    memset(&s, 0, sizeof s);
    s.rounds = fs.rounds;
    s.max_level_used = fs.max_level_used;
    s.n_legs = fs.n_legs;
    s.n_legs_at_cap = fs.n_legs_at_cap;
    s.n_cps = fs.n_cps;
    s.n_blocked_first = fs.n_hit_first;
    s.n_blocked = (int64_t)rec.acc[2];
    s.first_blocked = rec.acc[1] == ~0ull ? -1 : (int64_t)rec.acc[1];
    s.n_no_candidate = (int64_t)cnt[C_NONE];
    s.n_dir_changes = (int64_t)cnt[C_CHANGES];
    s.max_dir_turn = (int64_t)cnt[C_TURN];
    cnt[C_ACC + 0] = rec.acc[0];   // the sample terms are the last round's own
    cnt[C_ACC + 3] = rec.acc[3];
    clr_summary_from(cnt + C_ACC, &s.final);

    if (leg_level_out) memcpy(leg_level_out, lv.data(), sizeof(int32_t) * lv.size());
    if (seg_dir_out) memcpy(seg_dir_out, seg_dir.data(), sizeof(int32_t) * (size_t)n_seg);
    if (blocked_out) memcpy(blocked_out, blocked.data(), (size_t)n_seg);
    B.b->set = true;
    B.b->h_valid = false;
    *spline_out = B.b.release();
    if (samples_out) *samples_out = B.samples.release();
    *sum = s;
    return WA_OK;
}
