// host_ticks.inc -- C ABI: wa_traj_axes_smooth, wa_traj_axes_limits and wa_traj_tick_axes, the tool poses at controller ticks (included by
// weldacs.hip inside extern "C").  The host checks the arguments and the integer inputs it is handed (axes, legs, times); everything
// else stays on the device, on the context's stream; the host reads ONE WaAxRec before it copies any output.
static WaAxRec ax_rec0()
{
    WaAxRec r;
    memset(&r, 0, sizeof r);
    r.first_blocked = ~0ull;
    r.min_limit_bits = 0xffffffffu;
    return r;
}

// the quantised axes as the device keeps them; false: a component outside -16384 .. 16384 or an all-zero triple
static bool ax_pack(const int32_t *q, int64_t n, std::vector<short4> *out)
{
    out->resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t *v = q + 3 * (size_t)i;
        for (int c = 0; c < 3; c++)
            if (v[c] < -16384 || v[c] > 16384) return false;
        if (!v[0] && !v[1] && !v[2]) return false;
        (*out)[(size_t)i] = make_short4((short)v[0], (short)v[1], (short)v[2], 0);
    }
    return true;
}

// rint(x * 2^30) for a finite x >= 0 whose quanta stay at or below 2^61
static bool ax_quanta(double x, long long *out)
{
    if (!std::isfinite(x) || x < 0.0) return false;
    const double q = rint(x * WA_RT_Q);
    if (!(q <= (double)WA_RT_CAP)) return false;
    *out = (long long)q;
    return true;
}

int wa_traj_axes_smooth(const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, const int64_t *off, int32_t n_legs,
                        double h, int32_t max_level, int32_t *q_out, uint8_t *level_out, uint8_t *blocked_out, wa_axes_smooth_summary *sum)
{
    WaDevGuard dev_guard_(t ? t->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!t) return WA_ERR_ARG;
    wa_ctx *ctx = t->ctx;
    if (!q || !off || !q_out || !sum) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: NULL argument");
    if ((g == nullptr) != (tool == nullptr)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: a grid and a tool come together or not at all");
    if (g && g->ctx != ctx) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: trajectory and grid belong to different contexts");
    const int64_t n = t->n;
    if (n < 1 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: a trajectory needs 1 .. 2^31 samples");
    if (max_level < 0 || max_level > WA_AX_MAX_LEVEL) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: max_level must be 0 .. 8");
    long long h_q = 0;
    if (!ax_quanta(h, &h_q)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: h must be finite, >= 0 and at most 2^31");
    if (n_legs < 1) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: at least one leg");
    if (off[0] != 0 || off[n_legs] != n) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: off must run from 0 to the number of samples");
    bool long_leg = false;
    for (int32_t l = 0; l < n_legs; l++) {
        if (off[l + 1] < off[l]) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: off must not decrease");
        long_leg |= off[l + 1] - off[l] > ((int64_t)1 << 22);
    }
    WaTorchTool dt;
    if (tool && !torch_tool_dev(tool, -1, &dt)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: n_beads, dist16 or r2 out of range");
    std::vector<short4> hq;
    if (!ax_pack(q, n, &hq)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: an axis component outside -16384 .. 16384 or an all-zero axis");
    if (long_leg) return fail(ctx, WA_ERR_CAPACITY, "wa_traj_axes_smooth: a leg holds more than 2^22 samples");
    WaField F = {};
    if (g) {
        int rc = grid_field(g, &F);
        if (rc) return rc;
    }
    DevBuf<short4> dq, dq_out;
    DevBuf<uint8_t> dlevel, dblocked;
    DevBuf<long long> doff;
    DevBuf<WaTorchTool> dtool;
    DevBuf<WaAxRec> drec;
    CtxBuf<long long> dL(ctx), dGL(ctx);   // the scans' arrays and scratch: blocks of the context's arena
    CtxBuf<Ax3> dP(ctx), dscr3(ctx);
    CtxBuf<RtPair> dscr(ctx);
    CtxBuf<unsigned int> dlist(ctx);
    hipError_t e = dq.alloc((size_t)n);
    e = e ? e : dq_out.alloc((size_t)n);
    e = e ? e : dlevel.alloc((size_t)n);
    e = e ? e : dblocked.alloc((size_t)n);
    e = e ? e : doff.alloc((size_t)n_legs + 1);
    e = e ? e : drec.alloc(1);
    if (tool) e = e ? e : dtool.alloc(1);
    e = e ? e : dL.alloc((size_t)n);
    e = e ? e : dGL.alloc((size_t)n);
    e = e ? e : dP.alloc((size_t)n);
    e = e ? e : dscr3.alloc((size_t)wa_scan_scratch(n));
    e = e ? e : dscr.alloc((size_t)wa_scan_scratch(n));
    e = e ? e : dlist.alloc((size_t)n);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_traj_axes_smooth: device buffers");
    hipStream_t st = ctx->stream;
    WaAxRec rec = ax_rec0();
    e = hipMemcpyAsync(dq, hq.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(doff, off, sizeof(long long) * ((size_t)n_legs + 1), hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(drec, &rec, sizeof rec, hipMemcpyHostToDevice, st);
    if (tool) e = e ? e : hipMemcpyAsync(dtool, &dt, sizeof dt, hipMemcpyHostToDevice, st);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (e == hipSuccess) {
        k_ax_lengths<<<blocks, 256, 0, st>>>(t->xyz, n, dL, drec);
        e = hipGetLastError();
    }
    const RtSamples len = {dL, nullptr, dGL, n, 0};
    const Ax3Samples axes = {dq, dP, n};
    e = e ? e : wa_scan(st, len, dscr);
    e = e ? e : wa_scan(st, axes, dscr3);
    WaAxSmooth A;
    A.xyz = t->xyz; A.q = dq; A.GL = dGL; A.P = dP; A.off = doff; A.n = n; A.h_q = h_q; A.n_legs = n_legs; A.max_level = max_level;
    A.check = g ? 1 : 0; A.q_out = dq_out; A.level = dlevel; A.blocked = dblocked; A.list = dlist;
    if (e == hipSuccess) {
        k_ax_level0<<<blocks, 256, 0, st>>>(A, F, dtool, drec);
        if (g && max_level > 0) k_ax_climb<<<blocks, 256, 0, st>>>(A, F, dtool, drec);   // (blocks past the compacted count leave at once)
        k_ax_summary<<<blocks, 256, 0, st>>>(A, drec);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_axes_smooth: %s", hipGetErrorString(e));
    if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: a coordinate of the trajectory is not finite");
    int64_t length_q = 0;
    if (!rt_sum_fits(rec.sumL, &length_q)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_smooth: the sum of L reaches 2^61 quanta");
    // (every WA_ERR_ARG has been answered by now: nothing was written before this line)
    hq.resize((size_t)n);
    e = hipMemcpyAsync(hq.data(), dq_out, sizeof(short4) * (size_t)n, hipMemcpyDeviceToHost, st);
    if (level_out) e = e ? e : hipMemcpyAsync(level_out, dlevel, (size_t)n, hipMemcpyDeviceToHost, st);
    if (blocked_out) e = e ? e : hipMemcpyAsync(blocked_out, dblocked, (size_t)n, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_axes_smooth: %s", hipGetErrorString(e));
    for (int64_t i = 0; i < n; i++) {
        q_out[3 * i] = hq[(size_t)i].x;
        q_out[3 * i + 1] = hq[(size_t)i].y;
        q_out[3 * i + 2] = hq[(size_t)i].z;
    }
    wa_axes_smooth_summary s;
    memset(&s, 0, sizeof s);
    s.n = n;
    s.n_outside = (int64_t)rec.n_outside;
    for (int l = 0; l <= WA_AX_MAX_LEVEL; l++) s.n_level[l] = (int64_t)rec.n_level[l];
    s.n_blocked = (int64_t)rec.n_blocked;
    s.first_blocked = rec.first_blocked == ~0ull ? -1 : (int64_t)rec.first_blocked;
    s.n_zero_sum = (int64_t)rec.n_zero_sum;
    s.max_turn_in = (int64_t)rec.max_turn_in;
    s.max_turn_out = (int64_t)rec.max_turn_out;
    *sum = s;
    return WA_OK;
}

int wa_traj_axes_limits(const wa_traj *t, const int32_t *q, double omega, double v_cap, double v_floor, const float *v_limit_in,
                        float *v_limit_out, wa_axes_limits_summary *sum)
{
    WaDevGuard dev_guard_(t ? t->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!t) return WA_ERR_ARG;
    wa_ctx *ctx = t->ctx;
    if (!q || !v_limit_out || !sum) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: NULL argument");
    const int64_t n = t->n;
    if (n < 1 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: a trajectory needs 1 .. 2^31 samples");
    if (!rt_pos_finite(omega) || !rt_pos_finite(v_cap) || !rt_pos_finite(v_floor) || v_floor > v_cap)
        return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: omega, v_cap and v_floor must be finite and > 0, v_floor at most v_cap");
    float floor_f = (float)v_floor;   // the smallest float >= v_floor
    if ((double)floor_f < v_floor) floor_f = nextafterf(floor_f, INFINITY);
    if (!std::isfinite(floor_f)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: v_floor does not fit a float");
    std::vector<short4> hq;
    if (!ax_pack(q, n, &hq)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: an axis component outside -16384 .. 16384 or an all-zero axis");
    DevBuf<short4> dq;
    DevBuf<float> din, dout;
    DevBuf<WaAxRec> drec;
    hipError_t e = dq.alloc((size_t)n);
    e = e ? e : dout.alloc((size_t)n);
    e = e ? e : drec.alloc(1);
    if (v_limit_in) e = e ? e : din.alloc((size_t)n);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_traj_axes_limits: device buffers");
    hipStream_t st = ctx->stream;
    WaAxRec rec = ax_rec0();
    e = hipMemcpyAsync(dq, hq.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(drec, &rec, sizeof rec, hipMemcpyHostToDevice, st);
    if (v_limit_in) e = e ? e : hipMemcpyAsync(din, v_limit_in, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        k_ax_limits<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t->xyz, dq, n, omega, v_cap, v_floor, floor_f, din, dout, drec);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_axes_limits: %s", hipGetErrorString(e));
    if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: a coordinate of the trajectory is not finite");
    if (rec.bad & 4) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_limits: v_limit_in entries must be finite and > 0");
    e = hipMemcpyAsync(v_limit_out, dout, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_axes_limits: %s", hipGetErrorString(e));
    wa_axes_limits_summary s;
    memset(&s, 0, sizeof s);
    s.n = n;
    s.n_turning = (int64_t)rec.n_turning;
    s.n_jump = (int64_t)rec.n_jump;
    s.n_floored = (int64_t)rec.n_floored;
    s.n_limited = (int64_t)rec.n_limited;
    float mf;
    memcpy(&mf, &rec.min_limit_bits, sizeof mf);
    s.min_limit = (double)mf;
    *sum = s;
    return WA_OK;
}

// One driver for wa_traj_tick_axes and wa_traj_tick_axes_stops (host_stops.inc): stops == nullptr launches k_tk_axes as ever, otherwise
// k_tk_axes_stops with the segment tags and the second record.
static int tick_axes_run(const char *who, const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, int32_t near_add,
                         double acc, double dec, double tick, const int64_t *time_q, const int64_t *w_q, const uint8_t *seg_tag,
                         wa_traj **axes_out, uint8_t *blocked_out, uint8_t *tag_out, wa_tick_axes_summary *sum, wa_tick_stops_summary *stops)
{
    WaDevGuard dev_guard_(t ? t->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!t) return WA_ERR_ARG;
    wa_ctx *ctx = t->ctx;
    if (!q || !time_q || !w_q || !sum) return fail(ctx, WA_ERR_ARG, "%s: NULL argument", who);
    if ((g == nullptr) != (tool == nullptr)) return fail(ctx, WA_ERR_ARG, "%s: a grid and a tool come together or not at all", who);
    if (g && g->ctx != ctx) return fail(ctx, WA_ERR_ARG, "%s: trajectory and grid belong to different contexts", who);
    const int64_t n = t->n;
    if (n < 2 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "%s: a trajectory needs 2 .. 2^31 samples", who);
    if (!rt_pos_finite(acc) || !rt_pos_finite(dec)) return fail(ctx, WA_ERR_ARG, "%s: acc and dec must be finite and > 0", who);
    if (!std::isfinite(tick)) return fail(ctx, WA_ERR_ARG, "%s: tick must be finite", who);
    const double tq = rint(tick * WA_RT_Q);
    if (!(tq >= 1.0 && tq <= (double)WA_RT_CAP)) return fail(ctx, WA_ERR_ARG, "%s: tick must be 2^-30 .. 2^31 seconds", who);
    const long long tick_q = (long long)tq;
    if (time_q[0] != 0) return fail(ctx, WA_ERR_ARG, "%s: time_q must begin at 0", who);
    for (int64_t i = 0; i < n; i++) {
        if (time_q[i] >= WA_RT_CAP || (i > 0 && time_q[i] < time_q[i - 1]))
            return fail(ctx, WA_ERR_ARG, "%s: time_q must not decrease and stay below 2^61", who);
        if (w_q[i] < 0 || w_q[i] > WA_RT_CAP) return fail(ctx, WA_ERR_ARG, "%s: w_q must be 0 .. 2^61", who);
    }
    WaTorchTool dt;
    if (tool && !torch_tool_dev(tool, near_add, &dt)) return fail(ctx, WA_ERR_ARG, "%s: n_beads, dist16, r2 or near_add out of range", who);
    std::vector<short4> hq;
    if (!ax_pack(q, n, &hq)) return fail(ctx, WA_ERR_ARG, "%s: an axis component outside -16384 .. 16384 or an all-zero axis", who);
    WaField F = {};
    if (g) {
        int rc = grid_field(g, &F);
        if (rc) return rc;
    }
    const long long total = time_q[n - 1], n_full = total / tick_q + 1, n_ticks = n_full + (total % tick_q ? 1 : 0);
    const bool too_many = n_ticks > ((int64_t)1 << 31);
    DevBuf<short4> dq;
    DevBuf<long long> dB, dtime, dL;
    DevBuf<uint8_t> dblocked, dseg_tag, dtag;
    DevBuf<WaTorchTool> dtool;
    DevBuf<WaAxRec> drec;
    DevBuf<WaTkStopsRec> dsrec;
    OwnedHandle<wa_traj> axes;
    hipError_t e = dq.alloc((size_t)n);
    e = e ? e : dB.alloc((size_t)n);
    e = e ? e : dtime.alloc((size_t)n);
    e = e ? e : dL.alloc((size_t)n);
    e = e ? e : drec.alloc(1);
    if (tool) e = e ? e : dtool.alloc(1);
    if (blocked_out && !too_many) e = e ? e : dblocked.alloc((size_t)n_ticks);
    if (stops) e = e ? e : dsrec.alloc(1);
    if (seg_tag) e = e ? e : dseg_tag.alloc((size_t)n - 1);
    if (tag_out && !too_many) e = e ? e : dtag.alloc((size_t)n_ticks);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers", who);
    if (axes_out && !too_many) {
        wa_traj *a = nullptr;
        int rc = traj_alloc(ctx, n_ticks, &a);
        if (rc) return rc;
        axes.reset(a);
    }
    hipStream_t st = ctx->stream;
    WaAxRec rec = ax_rec0();
    e = hipMemcpyAsync(dq, hq.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(dB, w_q, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(dtime, time_q, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(drec, &rec, sizeof rec, hipMemcpyHostToDevice, st);
    if (tool) e = e ? e : hipMemcpyAsync(dtool, &dt, sizeof dt, hipMemcpyHostToDevice, st);
    if (stops) e = e ? e : hipMemsetAsync(dsrec, 0, sizeof(WaTkStopsRec), st);
    if (seg_tag) e = e ? e : hipMemcpyAsync(dseg_tag, seg_tag, (size_t)n - 1, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        k_ax_lengths<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t->xyz, n, dL, drec);   // (here for the coordinates that are not finite)
        e = hipGetLastError();
    }
    if (e == hipSuccess && !too_many) {
        WaTkArgs T;
        T.xyz = t->xyz; T.q = dq; T.B = dB; T.time_q = dtime; T.n = n; T.tick_q = tick_q; T.n_full = n_full; T.n_ticks = n_ticks;
        T.acc = acc; T.dec = dec; T.check = g ? 1 : 0; T.axes = axes ? axes->xyz : nullptr; T.blocked = dblocked;
        if (stops) {
            const WaTkStops S = {dseg_tag, dtag, dsrec};
            k_tk_axes_stops<<<(unsigned)((n_ticks + 255) / 256), 256, 0, st>>>(T, F, dtool, drec, S);
        } else {
            k_tk_axes<<<(unsigned)((n_ticks + 255) / 256), 256, 0, st>>>(T, F, dtool, drec);
        }
        e = hipGetLastError();
    }
    WaTkStopsRec srec;
    memset(&srec, 0, sizeof srec);
    e = e ? e : hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
    if (stops) e = e ? e : hipMemcpyAsync(&srec, dsrec, sizeof srec, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "%s: a coordinate of the trajectory is not finite", who);
    // (every WA_ERR_ARG has been answered by now: nothing was written before this line)
    if (too_many) {
        if (axes_out) *axes_out = nullptr;
        return fail(ctx, WA_ERR_CAPACITY, "%s: more than 2^31 ticks", who);
    }
    if (blocked_out || tag_out) {
        if (blocked_out) e = hipMemcpyAsync(blocked_out, dblocked, (size_t)n_ticks, hipMemcpyDeviceToHost, st);
        if (tag_out) e = e ? e : hipMemcpyAsync(tag_out, dtag, (size_t)n_ticks, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    wa_tick_axes_summary s;
    memset(&s, 0, sizeof s);
    s.n_ticks = n_ticks;
    for (int k = 0; k < WA_AX_SLOTS; k++) {
        s.n_outside += (int64_t)rec.slot[k].n_outside;
        s.n_blocked += (int64_t)rec.slot[k].n_blocked;
        s.n_near += (int64_t)rec.slot[k].n_near;
    }
    s.first_blocked = rec.first_blocked == ~0ull ? -1 : (int64_t)rec.first_blocked;
    s.max_tick_turn = (int64_t)rec.max_tick_turn;
    if (stops) {
        wa_tick_stops_summary s2;
        memset(&s2, 0, sizeof s2);
        for (int k = 0; k < WA_AX_SLOTS; k++) {
            s2.n_dwell_ticks += (int64_t)srec.slot[k].n_dwell;
            s2.n_tagged += (int64_t)srec.slot[k].n_tagged;
        }
        s2.max_dwell_turn = (int64_t)srec.max_dwell_turn;
        *stops = s2;
    }
    if (axes_out) *axes_out = axes.release();
    *sum = s;
    return WA_OK;
}

int wa_traj_tick_axes(const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, int32_t near_add, double acc, double dec,
                      double tick, const int64_t *time_q, const int64_t *w_q, wa_traj **axes_out, uint8_t *blocked_out,
                      wa_tick_axes_summary *sum)
{
    return tick_axes_run("wa_traj_tick_axes", g, t, q, tool, near_add, acc, dec, tick, time_q, w_q, nullptr, axes_out, blocked_out, nullptr, sum,
                         nullptr);
}
