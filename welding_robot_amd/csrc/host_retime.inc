// host_retime.inc -- C ABI: wa_traj_retime and wa_traj_retime_stops, speed caps, ramps, stops and controller ticks along a sampled
// trajectory (included by weldacs.hip inside extern "C").  One driver serves both calls: with dwell == nullptr it launches what
// wa_traj_retime always launched, with a dwell array the two kernels that know a stop (stops_kernels.hpp) in their place.  Everything between the arguments and the results stays on the device, on the context's stream; the host reads
// ONE WaRtRec (sums, counters, what was refused), sizes the tick buffer from it and launches the ticks.
// wa_traj_retime_jerk (host_jerk.inc) is a third caller: jk != nullptr takes the stops path on lowered caps and extended dwells and puts
// its own tick stage in the place of k_rt_ticks; with jk == nullptr every launch below is what it was.
struct JerkRun;
static int jk_check(wa_ctx *ctx, const wa_retime_limits *lim, double tick, long long tick_q, JerkRun *jk);
static bool jk_prepare_dwells(wa_ctx *ctx, JerkRun *jk, int64_t n, bool have_dwell, std::vector<long long> &hdq);
static int jk_caps(wa_ctx *ctx, const wa_traj *t, const WaRtLimits &dl, const float *v_limit, const WaField &field, const long long *dq,
                   JerkRun &jk, RtPair *scratch, long long *C, uint8_t *kind, WaRtRec *rec, bool *done);
static int jk_groups(wa_ctx *ctx, long long n, const long long *dq, JerkRun &jk, RtPair *scratch, uint8_t *bound);
static int jk_ticks(wa_ctx *ctx, const wa_traj *t, double acc, double dec, const long long *B, const long long *time_q, const long long *dq,
                    long long tick_q, long long n_full, long long n_u, long long n_out, long long length_q, JerkRun &jk, float *out_xyz);
static long long jk_n_out(const JerkRun &jk, long long n_u);
static int jk_length_check(wa_ctx *ctx, const JerkRun &jk, int64_t length_q);
static hipError_t jk_copy_out(wa_ctx *ctx, long long n_out, JerkRun &jk, WaJkRec *host_rec);
static void jk_summary(JerkRun &jk, const WaJkRec &r, long long n_u, long long n_out);
struct RetimeBuffers {
    DevBuf<long long> A, D, C, F, B, T, time_q, dq;
    DevBuf<uint8_t> kind, bound;
    DevBuf<float> v_limit;
    DevBuf<RtPair> scratch;
    DevBuf<WaRtRec> rec;
    OwnedHandle<wa_traj> ticks;
};

static bool rt_sum_fits(const unsigned long long w[2], int64_t *out)
{
    const unsigned __int128 v = ((unsigned __int128)w[1] << 32) + w[0];
    if (v >= (unsigned __int128)WA_RT_CAP) return false;
    *out = (int64_t)v;
    return true;
}

static bool rt_pos_finite(double x) { return x > 0.0 && std::isfinite(x); }

static int retime_run(const char *who, const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit,
                      const double *dwell, double tick, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                      wa_retime_summary *sum, wa_stops_summary *stops, JerkRun *jk = nullptr)
{
    WaDevGuard dev_guard_(t ? t->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!t) return WA_ERR_ARG;
    wa_ctx *ctx = t->ctx;
    if (!lim || !sum) return fail(ctx, WA_ERR_ARG, "%s: NULL limits or summary", who);
    if (g && g->ctx != ctx) return fail(ctx, WA_ERR_ARG, "%s: trajectory and grid belong to different contexts", who);
    const int64_t n = t->n;
    if (n < 2 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "%s: a trajectory needs 2 .. 2^31 samples", who);
    if (!rt_pos_finite(lim->v_max) || !rt_pos_finite(lim->acc) || !rt_pos_finite(lim->dec))
        return fail(ctx, WA_ERR_ARG, "%s: v_max, acc and dec must be finite and > 0", who);
    if (!(lim->a_lat >= 0.0)) return fail(ctx, WA_ERR_ARG, "%s: a_lat must be >= 0 (0 or +inf: no curvature cap)", who);
    if (g && lim->near_d2 >= 0 && !rt_pos_finite(lim->v_near)) return fail(ctx, WA_ERR_ARG, "%s: v_near must be finite and > 0", who);
    if (!std::isfinite(tick)) return fail(ctx, WA_ERR_ARG, "%s: tick must be finite", who);
    const double tq = rint(tick * WA_RT_Q);
    if (!(tq >= 1.0 && tq <= (double)WA_RT_CAP)) return fail(ctx, WA_ERR_ARG, "%s: tick must be 2^-30 .. 2^31 seconds", who);
    const long long tick_q = (long long)tq;
    if (jk) {
        int rc = jk_check(ctx, lim, tick, tick_q, jk);
        if (rc) return rc;
    }
    std::vector<long long> hdq;   // rule 40: the dwells in quanta, -1 where the segment is no stop
    wa_stops_summary ss;
    memset(&ss, 0, sizeof ss);
    if (dwell) {
        hdq.resize((size_t)n - 1);
        for (int64_t i = 0; i < n - 1; i++) {
            if (!std::isfinite(dwell[i])) return fail(ctx, WA_ERR_ARG, "%s: dwell entries must be finite", who);
            const double dq = dwell[i] < 0.0 ? -1.0 : rint(dwell[i] * WA_RT_Q);
            if (!(dq < (double)WA_RT_CAP)) return fail(ctx, WA_ERR_ARG, "%s: a dwell reaches 2^61 quanta", who);
            hdq[(size_t)i] = (long long)dq;
            if (dq < 0.0) continue;
            ss.n_stops++;
            ss.n_stop_samples += (i == 0 || hdq[(size_t)i - 1] < 0) ? 2 : 1;   // (a sample between two stops counts once)
            ss.dwell_q = ss.dwell_q + (long long)dq < WA_RT_CAP ? ss.dwell_q + (long long)dq : WA_RT_CAP;   // (the device refuses such a sum)
        }
    }
    if (jk && !jk_prepare_dwells(ctx, jk, n, dwell != nullptr, hdq)) return WA_ERR_ARG;   // (rule 50: hdq extended, all -1 without a dwell array)
    const bool with_stops = dwell || jk;
    WaField field = {};   // (no grid: all zero)
    if (g) {
        int rc = grid_field(g, &field);
        if (rc) return rc;
    }

    RetimeBuffers R;
    hipError_t e = hipSuccess;
    for (DevBuf<long long> *b : {&R.A, &R.D, &R.C, &R.F, &R.B, &R.T, &R.time_q}) e = e ? e : b->alloc((size_t)n);
    e = e ? e : R.kind.alloc((size_t)n);
    e = e ? e : R.bound.alloc((size_t)n);
    e = e ? e : R.scratch.alloc((size_t)wa_scan_scratch(n));
    e = e ? e : R.rec.alloc(1);
    if (v_limit) e = e ? e : R.v_limit.alloc((size_t)n);
    if (with_stops) e = e ? e : R.dq.alloc((size_t)n - 1);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", who);
    e = hipMemsetAsync(R.rec, 0, sizeof(WaRtRec), ctx->stream);
    if (v_limit) e = e ? e : hipMemcpyAsync(R.v_limit, v_limit, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream);
    if (with_stops) e = e ? e : hipMemcpyAsync(R.dq, hdq.data(), sizeof(long long) * ((size_t)n - 1), hipMemcpyHostToDevice, ctx->stream);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    WaRtLimits dl;
    dl.v_max = lim->v_max; dl.acc = lim->acc; dl.dec = lim->dec; dl.a_lat = lim->a_lat; dl.v_near = lim->v_near;
    dl.near_d2 = g ? lim->near_d2 : -1;
    dl.curv = std::isfinite(lim->a_lat) && lim->a_lat != 0.0;
    if (e == hipSuccess) {
        k_rt_segments<<<blocks, 256, 0, ctx->stream>>>(t->xyz, n, dl.acc, dl.dec, R.A, R.D, R.rec);
        bool lowered = false;   // rule 49 has written C and kind
        if (jk) {
            int rc = jk_caps(ctx, t, dl, R.v_limit, field, R.dq, *jk, R.scratch, R.C, R.kind, R.rec, &lowered);
            if (rc) return rc;
        }
        if (lowered) {
        } else if (with_stops) k_st_caps<<<blocks, 256, 0, ctx->stream>>>(t->xyz, n, dl, R.v_limit, field, R.dq, R.C, R.kind, R.rec);
        else k_rt_caps<<<blocks, 256, 0, ctx->stream>>>(t->xyz, n, dl, R.v_limit, field, R.C, R.kind, R.rec);
        e = hipGetLastError();
    }
    const RtSamples fwd = {R.A, R.C, R.F, n, 0}, bwd = {R.D, R.F, R.B, n, 1}, tim = {R.T, nullptr, R.time_q, n, 0};
    e = e ? e : wa_scan(ctx->stream, fwd, R.scratch);
    e = e ? e : wa_scan(ctx->stream, bwd, R.scratch);
    if (e == hipSuccess) {
        if (with_stops) k_st_times<<<blocks, 256, 0, ctx->stream>>>(t->xyz, n, dl.acc, dl.dec, R.A, R.D, R.C, R.B, R.kind, R.dq, R.bound, R.T, R.rec);
        else k_rt_times<<<blocks, 256, 0, ctx->stream>>>(t->xyz, n, dl.acc, dl.dec, R.A, R.D, R.C, R.B, R.kind, R.bound, R.T, R.rec);
        e = hipGetLastError();
    }
    e = e ? e : wa_scan(ctx->stream, tim, R.scratch);
    if (jk && e == hipSuccess) {
        int rc = jk_groups(ctx, n, R.dq, *jk, R.scratch, R.bound);
        if (rc) return rc;
    }
    WaRtRec rec;
    e = e ? e : hipMemcpyAsync(&rec, R.rec, sizeof rec, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "%s: a coordinate of the trajectory is not finite", who);
    if (rec.bad & 4) return fail(ctx, WA_ERR_ARG, "%s: v_limit entries must be finite and > 0", who);   // (k_rt_caps looked at every entry)
    if (rec.bad & 8) return fail(ctx, WA_ERR_ARG, "%s: a stop sits on a segment that has a length", who);
    wa_retime_summary s;
    memset(&s, 0, sizeof s);
    int64_t sum_a = 0, sum_d = 0;
    if (!rt_sum_fits(rec.sumL, &s.length_q) || !rt_sum_fits(rec.sumA, &sum_a) || !rt_sum_fits(rec.sumD, &sum_d))
        return fail(ctx, WA_ERR_ARG, "%s: the sum of L, A or D reaches 2^61 quanta", who);
    if ((rec.bad & 2) || !rt_sum_fits(rec.sumT, &s.time_q)) return fail(ctx, WA_ERR_ARG, "%s: the duration reaches 2^61 quanta", who);
    s.n = n;
    const long long n_full = s.time_q / tick_q + 1;
    s.n_ticks = n_full + (s.time_q % tick_q ? 1 : 0);
    for (int k = 0; k < 4; k++) s.n_bound[k] = (int64_t)rec.n_bound[k];
    s.n_on_cap = (int64_t)rec.n_on_cap;
    s.n_on_ramp = (int64_t)rec.n_on_ramp;
    s.n_triangle = (int64_t)rec.n_triangle;
    s.n_outside = (int64_t)rec.n_outside;
    s.peak_w_q = rec.peak;
    const long long n_out = jk ? jk_n_out(*jk, s.n_ticks) : s.n_ticks;   // (rule 53: W - 1 more)
    if (jk) {
        int rc = jk_length_check(ctx, *jk, s.length_q);
        if (rc) return rc;
    }
    const bool too_many = n_out > ((int64_t)1 << 31);
    if (ticks_out && !too_many) {
        wa_traj *ticks = nullptr;
        int rc = traj_alloc(ctx, n_out, &ticks);
        if (rc) return rc;
        R.ticks.reset(ticks);
    }
    if (jk) {
        if (!too_many) {
            int rc = jk_ticks(ctx, t, dl.acc, dl.dec, R.B, R.time_q, R.dq, tick_q, n_full, s.n_ticks, n_out, s.length_q, *jk,
                              R.ticks ? R.ticks->xyz : nullptr);
            if (rc) return rc;
        }
    } else if (R.ticks) {
        k_rt_ticks<<<(unsigned)((s.n_ticks + 255) / 256), 256, 0, ctx->stream>>>(t->xyz, n, dl.acc, dl.dec, R.B, R.time_q, tick_q, n_full,
                                                                                 s.n_ticks, R.ticks->xyz);
        e = hipGetLastError();
    }
    // (every WA_ERR_ARG has been answered by now: nothing was written before this line)
    if (time_q_out) e = e ? e : hipMemcpyAsync(time_q_out, R.time_q, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (w_q_out) e = e ? e : hipMemcpyAsync(w_q_out, R.B, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (bound_out) e = e ? e : hipMemcpyAsync(bound_out, R.bound, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    WaJkRec jrec = {};
    if (jk) e = e ? e : jk_copy_out(ctx, n_out, *jk, &jrec);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    if (ticks_out) *ticks_out = R.ticks.release();
    *sum = s;
    if (stops) *stops = ss;
    if (jk) jk_summary(*jk, jrec, s.n_ticks, n_out);
    if (too_many) return fail(ctx, WA_ERR_CAPACITY, "%s: more than 2^31 ticks", who);
    return WA_OK;
}

int wa_traj_retime(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, double tick,
                   int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out, wa_retime_summary *sum)
{
    return retime_run("wa_traj_retime", g, t, lim, v_limit, nullptr, tick, time_q_out, w_q_out, bound_out, ticks_out, sum, nullptr);
}

int wa_traj_retime_stops(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, const double *dwell,
                         double tick, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                         wa_retime_summary *sum, wa_stops_summary *stops)
{
    if (t && !stops) return fail(t->ctx, WA_ERR_ARG, "wa_traj_retime_stops: NULL stops summary");
    return retime_run("wa_traj_retime_stops", g, t, lim, v_limit, dwell, tick, time_q_out, w_q_out, bound_out, ticks_out, sum, stops);
}
