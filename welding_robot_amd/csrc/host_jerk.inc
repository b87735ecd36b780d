// host_jerk.inc -- C ABI: wa_traj_retime_jerk and wa_traj_jerk_window, jerk-limited controller ticks by a moving average along the arc
// length (included by weldacs.hip inside extern "C", behind host_retime.inc: retime_run is the driver, which declares the stages below
// and calls them for this call alone).  The profile is computed by the kernels of wa_traj_retime_stops on lowered caps and extended
// dwells; the host reads the window width (only when caps are lowered), then the ONE WaRtRec, sizes the tick buffers and launches the
// tick stage; the jerk record comes back with the outputs.
struct JerkRun;
struct JerkBuffers {
    DevBuf<long long> GL, next, P, s_q;
    DevBuf<unsigned long long> key, table, need, rest_cnt, first;   // first: per stop its lowest rest tick, with the axes only
    DevBuf<uint2> win;
    DevBuf<uint8_t> low, seg_tag, tag;
    DevBuf<WaJkRec> rec;
};
struct JerkAxesRun;   // host_jerk_axes.inc: what wa_traj_retime_jerk_axes adds, nullptr in a plain wa_traj_retime_jerk
static int jx_launch(wa_ctx *ctx, const WaJkTicks &T, long long n, const long long *dq, JerkRun &jk);
static hipError_t jx_copy_out(wa_ctx *ctx, long long n_out, JerkRun &jk);
static void jx_summary(JerkRun &jk, const WaJkRec &r, long long n_out, bool too_many);
struct JerkRun {
    const char *who;
    JerkAxesRun *ax;
    int32_t W;
    long long R_q, ext;         // rule 48's reach; (W - 1) * tick_q, what rule 50 adds to every dwell
    bool any_stop;
    const uint8_t *seg_tag;
    int64_t *s_q_out;
    uint8_t *tag_out;
    wa_jerk_summary *out;
    JerkBuffers J;
};

// rule 48, what can be said from the arguments alone
static int jk_check(wa_ctx *ctx, const wa_retime_limits *lim, double tick, long long tick_q, JerkRun *jk)
{
    const double step = floor((lim->v_max * tick) * WA_RT_Q);
    if (!(step < (double)WA_RT_CAP)) return fail(ctx, WA_ERR_ARG, "%s: v_max * tick reaches 2^61 quanta", jk->who);
    const unsigned __int128 reach = (unsigned __int128)(jk->W - 1) * (unsigned __int128)((long long)step + 1);
    const unsigned __int128 ext = (unsigned __int128)(jk->W - 1) * (unsigned __int128)tick_q;
    if (reach >= (unsigned __int128)WA_RT_CAP || ext >= (unsigned __int128)WA_RT_CAP)
        return fail(ctx, WA_ERR_ARG, "%s: the window's reach or time reaches 2^61 quanta", jk->who);
    jk->R_q = (long long)reach;
    jk->ext = (long long)ext;
    return WA_OK;
}

// rule 50: every dwell extended by (W - 1) * tick_q; a call without a dwell array takes the stops path with no stop in it
static bool jk_prepare_dwells(wa_ctx *ctx, JerkRun *jk, int64_t n, bool have_dwell, std::vector<long long> &hdq)
{
    if (!have_dwell) hdq.assign((size_t)n - 1, -1);
    jk->any_stop = false;
    for (long long &d : hdq) {
        if (d < 0) continue;
        if (d + jk->ext >= WA_RT_CAP) {
            fail(ctx, WA_ERR_ARG, "%s: an extended dwell reaches 2^61 quanta", jk->who);
            return false;
        }
        d += jk->ext;
        jk->any_stop = true;
    }
    return true;
}
static long long jk_n_out(const JerkRun &jk, long long n_u) { return n_u + jk.W - 1; }
static int jk_length_check(wa_ctx *ctx, const JerkRun &jk, int64_t length_q)
{
    if ((unsigned __int128)jk.W * (unsigned __int128)length_q >= ((unsigned __int128)1 << 62))
        return fail(ctx, WA_ERR_ARG, "%s: window * length reaches 2^62 quanta", jk.who);
    return WA_OK;
}

// GL, and with R_q > 0 rules 49 and 2: C and kind as k_st_caps leaves them, from lowered caps.  rec is the call's zeroed WaRtRec.
static int jk_caps(wa_ctx *ctx, const wa_traj *t, const WaRtLimits &dl, const float *v_limit, const WaField &field, const long long *dq,
                   JerkRun &jk, RtPair *scratch, long long *C, uint8_t *kind, WaRtRec *rec, bool *done)
{
    JerkBuffers &J = jk.J;
    const long long n = t->n;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipError_t e = J.GL.alloc((size_t)n);
    e = e ? e : J.rec.alloc(1);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", jk.who);
    e = hipMemsetAsync(J.rec, 0, sizeof(WaJkRec), ctx->stream);
    const JkLengths len = {t->xyz, J.GL, n};
    e = e ? e : wa_scan(ctx->stream, len, scratch);
    *done = false;
    if (e == hipSuccess && jk.R_q > 0) {
        e = J.key.alloc((size_t)n);
        e = e ? e : J.win.alloc((size_t)n);
        e = e ? e : J.low.alloc((size_t)n);
        if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", jk.who);
        k_jk_caps<<<blocks, 256, 0, ctx->stream>>>(t->xyz, n, dl, v_limit, field, (long long *)J.key.p, rec);
        k_jk_window<<<blocks, 256, 0, ctx->stream>>>(J.GL, n, jk.R_q, J.win, J.rec);
        e = hipGetLastError();
        // the widest window sizes the table; the sum of L is complete by now, and GL means nothing where it reaches 2^61
        WaJkRec jr;
        WaRtRec rr;
        e = e ? e : hipMemcpyAsync(&jr, J.rec, sizeof jr, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(&rr, rec, sizeof rr, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", jk.who, hipGetErrorString(e));
        int64_t length_q = 0;
        if (rr.bad & 1) return fail(ctx, WA_ERR_ARG, "%s: a coordinate of the trajectory is not finite", jk.who);
        if (!rt_sum_fits(rr.sumL, &length_q)) return fail(ctx, WA_ERR_ARG, "%s: the sum of L, A or D reaches 2^61 quanta", jk.who);
        int levels = 0;
        while ((2ull << levels) <= jr.max_width) levels++;   // floor(log2(width)) of the widest window
        if (levels) {
            if (J.table.alloc((size_t)levels * (size_t)n) != hipSuccess)
                return fail(ctx, WA_ERR_ALLOC, "%s: the table of range minima (8 n bytes per level)", jk.who);
            for (int l = 1; l <= levels; l++)
                k_jk_level<<<blocks, 256, 0, ctx->stream>>>(l == 1 ? J.key.p : J.table.p + (size_t)(l - 2) * n, J.table.p + (size_t)(l - 1) * n, n,
                                                            1ll << (l - 1));
        }
        k_jk_lower<<<blocks, 256, 0, ctx->stream>>>(J.key, J.table, n, J.win, dq, C, kind, J.low, J.rec);
        e = hipGetLastError();
        *done = true;
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", jk.who, hipGetErrorString(e));
    return WA_OK;
}

// behind k_st_times: bit 6 of bound, the next stop of every sample, the dwell every group of stops was given
static int jk_groups(wa_ctx *ctx, long long n, const long long *dq, JerkRun &jk, RtPair *scratch, uint8_t *bound)
{
    JerkBuffers &J = jk.J;
    hipError_t e = hipSuccess;
    if (jk.any_stop) {
        e = J.next.alloc((size_t)n);
        e = e ? e : J.need.alloc((size_t)n);
        e = e ? e : J.rest_cnt.alloc((size_t)n);
        if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", jk.who);
        e = hipMemsetAsync(J.need, 0, sizeof(unsigned long long) * n, ctx->stream);
        e = e ? e : hipMemsetAsync(J.rest_cnt, 0, sizeof(unsigned long long) * n, ctx->stream);
        const JkNext nx = {dq, J.next, n};
        e = e ? e : wa_scan(ctx->stream, nx, scratch);
    }
    if (e == hipSuccess && (jk.any_stop || J.low.p)) {
        k_jk_groups<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(J.GL, n, J.low, dq, J.next, jk.ext, bound, J.need);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", jk.who, hipGetErrorString(e));
    return WA_OK;
}

// rules 52 - 55 behind the record: the arc lengths, their prefix sums, the output ticks.  n_u unfiltered ticks, n_out = n_u + W - 1.
static int jk_ticks(wa_ctx *ctx, const wa_traj *t, double acc, double dec, const long long *B, const long long *time_q, const long long *dq,
                    long long tick_q, long long n_full, long long n_u, long long n_out, long long length_q, JerkRun &jk, float *out_xyz)
{
    JerkBuffers &J = jk.J;
    const long long n = t->n;
    hipError_t e = J.P.alloc((size_t)n_u + 1);
    DevBuf<RtPair> scratch;
    e = e ? e : scratch.alloc((size_t)wa_scan_scratch(n_u + 1));
    if (jk.s_q_out) e = e ? e : J.s_q.alloc((size_t)n_out);
    if (jk.tag_out) {
        e = e ? e : J.tag.alloc((size_t)n_out);
        e = e ? e : J.seg_tag.alloc((size_t)n - 1);
    }
    if (jk.ax && jk.any_stop) e = e ? e : J.first.alloc((size_t)n);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: tick buffers", jk.who);
    if (J.first.p) e = hipMemsetAsync(J.first, 0xff, sizeof(unsigned long long) * n, ctx->stream);   // (a minimum: ~0 where no tick rests)
    if (jk.tag_out) e = e ? e : hipMemcpyAsync(J.seg_tag, jk.seg_tag, (size_t)n - 1, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        k_jk_arcs<<<(unsigned)((n_u + 255) / 256), 256, 0, ctx->stream>>>(t->xyz, n, acc, dec, B, time_q, J.GL, tick_q, n_full, n_u, J.P);
        e = hipGetLastError();
    }
    const RtSamples sums = {J.P, nullptr, J.P, n_u + 1, 0};   // (in place: a lane has read its eight entries before it writes them)
    e = e ? e : wa_scan(ctx->stream, sums, scratch);
    if (e == hipSuccess) {
        WaJkTicks T;
        T.xyz = t->xyz; T.n = n; T.GL = J.GL; T.next = J.next; T.P = J.P; T.n_u = n_u; T.n_ticks = n_out; T.length_q = length_q;
        T.W = (unsigned long long)jk.W; T.seg_tag = jk.tag_out ? J.seg_tag.p : nullptr; T.out = out_xyz; T.s_q = J.s_q; T.tag = J.tag;
        T.rest_cnt = J.rest_cnt; T.rec = J.rec;
        if (jk.ax && jk.any_stop) k_jk_ticks_first<<<(unsigned)((n_out + 255) / 256), 256, 0, ctx->stream>>>(T, J.first);
        else k_jk_ticks<<<(unsigned)((n_out + 255) / 256), 256, 0, ctx->stream>>>(T);
        if (jk.any_stop)
            k_jk_rests<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(J.GL, n, dq, J.next, J.need, J.rest_cnt, (unsigned long long)tick_q, J.rec);
        e = hipGetLastError();
        if (jk.ax && e == hipSuccess) {   // rules 57 - 60 behind the counts of every stop
            int rc = jx_launch(ctx, T, n, dq, jk);
            if (rc) return rc;
        }
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", jk.who, hipGetErrorString(e));
    return WA_OK;
}

// the outputs of this call alone, enqueued with the per-sample copies; the summary behind the synchronisation
static hipError_t jk_copy_out(wa_ctx *ctx, long long n_out, JerkRun &jk, WaJkRec *host_rec)
{
    hipError_t e = hipMemcpyAsync(host_rec, jk.J.rec, sizeof(WaJkRec), hipMemcpyDeviceToHost, ctx->stream);
    if (jk.s_q_out && jk.J.s_q.p) e = e ? e : hipMemcpyAsync(jk.s_q_out, jk.J.s_q, sizeof(int64_t) * n_out, hipMemcpyDeviceToHost, ctx->stream);
    if (jk.tag_out && jk.J.tag.p) e = e ? e : hipMemcpyAsync(jk.tag_out, jk.J.tag, (size_t)n_out, hipMemcpyDeviceToHost, ctx->stream);
    if (jk.ax) e = e ? e : jx_copy_out(ctx, n_out, jk);
    return e;
}
// (above 2^31 ticks the tick stage did not run: its fields of the zeroed record are 0)
static void jk_summary(JerkRun &jk, const WaJkRec &r, long long n_u, long long n_out)
{
    if (jk.ax) jx_summary(jk, r, n_out, n_out > ((int64_t)1 << 31));
    wa_jerk_summary s;
    memset(&s, 0, sizeof s);
    s.window = jk.W;
    s.reach_q = jk.R_q;
    s.n_lowered = (int64_t)r.n_lowered;
    s.n_in = n_u;
    s.n_ticks = n_out;
    s.max_d1 = (int64_t)r.max_d1;
    s.max_d2 = (int64_t)r.max_d2;
    s.max_d3 = (int64_t)r.max_d3;
    s.in_max_d2 = (int64_t)r.in_max_d2;
    s.n_rest_ticks = (int64_t)r.n_rest;
    s.n_short_rests = (int64_t)r.n_short;
    s.n_back = (int64_t)r.n_back;
    *jk.out = s;
}

// One body for wa_traj_retime_jerk and wa_traj_retime_jerk_axes (host_jerk_axes.inc): ax == nullptr enqueues what wa_traj_retime_jerk
// always enqueued.
static int jerk_run(const char *who, const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, const double *dwell,
                    double tick, int32_t window, const uint8_t *seg_tag, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out,
                    wa_traj **ticks_out, int64_t *s_q_out, uint8_t *tag_out, wa_retime_summary *sum, wa_stops_summary *stops,
                    wa_jerk_summary *jerk, JerkAxesRun *ax)
{
    if (!t) return WA_ERR_ARG;
    if (!stops || !jerk) return fail(t->ctx, WA_ERR_ARG, "%s: NULL stops or jerk summary", who);
    if (window < 1 || window > WA_JK_MAX_W) return fail(t->ctx, WA_ERR_ARG, "%s: the window must be 1 .. 2^20 ticks", who);
    if (tag_out && !seg_tag) return fail(t->ctx, WA_ERR_ARG, "%s: tag_out without seg_tag", who);
    JerkRun jk = {};
    jk.who = who;
    jk.ax = ax;
    jk.W = window;
    jk.seg_tag = seg_tag;
    jk.s_q_out = s_q_out;
    jk.tag_out = tag_out;
    jk.out = jerk;
    return retime_run(who, g, t, lim, v_limit, dwell, tick, time_q_out, w_q_out, bound_out, ticks_out, sum, stops, &jk);
}

int wa_traj_retime_jerk(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, const double *dwell,
                        double tick, int32_t window, const uint8_t *seg_tag, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out,
                        wa_traj **ticks_out, int64_t *s_q_out, uint8_t *tag_out, wa_retime_summary *sum, wa_stops_summary *stops,
                        wa_jerk_summary *jerk)
{
    return jerk_run("wa_traj_retime_jerk", g, t, lim, v_limit, dwell, tick, window, seg_tag, time_q_out, w_q_out, bound_out, ticks_out, s_q_out,
                    tag_out, sum, stops, jerk, nullptr);
}

int wa_traj_jerk_window(const wa_traj *t, double acc, double dec, double jerk, double tick, int32_t *window_out)
{
    wa_ctx *ctx = t ? t->ctx : nullptr;
    if (!window_out || !rt_pos_finite(acc) || !rt_pos_finite(dec) || !rt_pos_finite(jerk) || !rt_pos_finite(tick))
        return fail(ctx, WA_ERR_ARG, "wa_traj_jerk_window: acc, dec, jerk and tick must be finite and > 0, window_out not NULL");
    const double w = ceil((2.0 * (acc > dec ? acc : dec)) / (jerk * tick));
    if (!(w <= (double)WA_JK_MAX_W)) return fail(ctx, WA_ERR_ARG, "wa_traj_jerk_window: the window exceeds 2^20 ticks");
    *window_out = w < 1.0 ? 1 : (int32_t)w;
    return WA_OK;
}
