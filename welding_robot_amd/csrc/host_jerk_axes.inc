// host_jerk_axes.inc -- C ABI: wa_traj_retime_jerk_axes, the torch axes at jerk-limited ticks (included by weldacs.hip inside extern "C",
// behind host_jerk.inc, host_torch.inc and host_ticks.inc).  The call is wa_traj_retime_jerk's body (jerk_run) with one more stage: the
// host checks the axes and the tool before anything is enqueued, jk_ticks launches k_jk_axes behind its own kernels while the prefix
// sums of the arc lengths are still on the device, and the two records come back with that call's outputs.
struct FramesRun;   // host_frames.inc: what wa_traj_retime_jerk_frames adds, nullptr in a plain wa_traj_retime_jerk_axes
static int fr_launch(wa_ctx *ctx, const WaJkTicks &T, long long n, const WaJkAxes &A, JerkRun &jk, FramesRun &Fr, const WaField &F,
                     const WaTorchTool *dtool, WaAxRec *drec);
static hipError_t fr_copy_out(wa_ctx *ctx, FramesRun &Fr);
static void fr_summary(FramesRun &Fr, long long n_out, bool too_many);
struct JerkAxesRun {
    FramesRun *fr;
    std::vector<short4> hq;   // the quantised axes, packed
    WaTorchTool tool;
    WaField F;
    bool check;               // a grid and a tool are given
    wa_traj **axes_out;
    uint8_t *blocked_out;
    wa_jerk_axes_summary *out;
    WaAxRec rec;
    WaJxRec xrec;
    DevBuf<short4> q;
    DevBuf<uint8_t> blocked;
    DevBuf<WaTorchTool> dtool;
    DevBuf<WaAxRec> drec;
    DevBuf<WaJxRec> dxrec;
    OwnedHandle<wa_traj> axes;
};

static WaJxRec jx_rec0()
{
    WaJxRec r;
    memset(&r, 0, sizeof r);
    r.min_turn_ticks = ~0ull;
    return r;
}

// rules 57 - 60 behind k_jk_ticks and k_jk_rests: T is what k_jk_ticks was given, n_ticks <= 2^31
static int jx_launch(wa_ctx *ctx, const WaJkTicks &T, long long n, const long long *dq, JerkRun &jk)
{
    JerkAxesRun &X = *jk.ax;
    hipStream_t st = ctx->stream;
    hipError_t e = X.q.alloc((size_t)n);
    e = e ? e : X.drec.alloc(1);
    e = e ? e : X.dxrec.alloc(1);
    if (X.check) e = e ? e : X.dtool.alloc(1);
    if (X.blocked_out) e = e ? e : X.blocked.alloc((size_t)T.n_ticks);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers of the axes", jk.who);
    if (X.axes_out) {
        wa_traj *a = nullptr;
        int rc = traj_alloc(ctx, T.n_ticks, &a);
        if (rc) return rc;
        X.axes.reset(a);
    }
    X.rec = ax_rec0();
    X.xrec = jx_rec0();
    e = hipMemcpyAsync(X.q, X.hq.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(X.drec, &X.rec, sizeof X.rec, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemcpyAsync(X.dxrec, &X.xrec, sizeof X.xrec, hipMemcpyHostToDevice, st);
    if (X.check) e = e ? e : hipMemcpyAsync(X.dtool, &X.tool, sizeof X.tool, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        WaJkAxes A;
        A.q = X.q; A.first = jk.J.first; A.check = X.check ? 1 : 0; A.axes = X.axes ? X.axes->xyz : nullptr; A.blocked = X.blocked;
        A.rec = X.dxrec;
        if (X.fr) {   // rules 61 - 67: the same body with the frames policy
            int rc = fr_launch(ctx, T, n, A, jk, *X.fr, X.F, X.dtool, X.drec);
            if (rc) return rc;
        } else {
            k_jk_axes<<<(unsigned)((T.n_ticks + 255) / 256), 256, 0, st>>>(T, A, X.F, X.dtool, X.drec);
        }
        if (jk.any_stop)
            k_jx_groups<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(jk.J.GL, n, dq, jk.J.next, X.q, jk.J.rest_cnt, X.dxrec);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", jk.who, hipGetErrorString(e));
    return WA_OK;
}

// (above 2^31 ticks the stage did not run: nothing to copy)
static hipError_t jx_copy_out(wa_ctx *ctx, long long n_out, JerkRun &jk)
{
    JerkAxesRun &X = *jk.ax;
    if (!X.drec.p) return hipSuccess;
    hipError_t e = hipMemcpyAsync(&X.rec, X.drec, sizeof X.rec, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipMemcpyAsync(&X.xrec, X.dxrec, sizeof X.xrec, hipMemcpyDeviceToHost, ctx->stream);
    if (X.blocked_out) e = e ? e : hipMemcpyAsync(X.blocked_out, X.blocked, (size_t)n_out, hipMemcpyDeviceToHost, ctx->stream);
    if (X.fr) e = e ? e : fr_copy_out(ctx, *X.fr);
    return e;
}

static void jx_summary(JerkRun &jk, const WaJkRec &r, long long n_out, bool too_many)
{
    JerkAxesRun &X = *jk.ax;
    wa_jerk_axes_summary s;
    memset(&s, 0, sizeof s);
    if (!too_many) {
        s.n_ticks = n_out;
        for (int k = 0; k < WA_AX_SLOTS; k++) {
            s.n_outside += (int64_t)X.rec.slot[k].n_outside;
            s.n_blocked += (int64_t)X.rec.slot[k].n_blocked;
            s.n_near += (int64_t)X.rec.slot[k].n_near;
        }
        s.first_blocked = X.rec.first_blocked == ~0ull ? -1 : (int64_t)X.rec.first_blocked;
        s.max_tick_turn = (int64_t)X.rec.max_tick_turn;
        s.n_rest_ticks = (int64_t)r.n_rest;
        s.n_turning_rests = (int64_t)X.xrec.n_turning;
        s.min_turn_ticks = X.xrec.min_turn_ticks == ~0ull ? 0 : (int64_t)X.xrec.min_turn_ticks;
        s.max_rest_turn = (int64_t)X.xrec.max_rest_turn;
    }
    if (X.axes_out) *X.axes_out = X.axes.release();   // (NULL above 2^31 ticks)
    *X.out = s;
    if (X.fr) fr_summary(*X.fr, n_out, too_many);
}

// One body for wa_traj_retime_jerk_axes and wa_traj_retime_jerk_frames (host_frames.inc): fr == nullptr enqueues what
// wa_traj_retime_jerk_axes always enqueued.
static int jerk_axes_run(const char *who, const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit,
                         const double *dwell, double tick, int32_t window, const uint8_t *seg_tag, const int32_t *q, const wa_tool_beads *tool,
                         int32_t near_add, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out, int64_t *s_q_out,
                         uint8_t *tag_out, wa_traj **axes_out, uint8_t *blocked_out, wa_retime_summary *sum, wa_stops_summary *stops,
                         wa_jerk_summary *jerk, wa_jerk_axes_summary *axes, FramesRun *fr)
{
    WaDevGuard dev_guard_(t ? t->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!t) return WA_ERR_ARG;
    wa_ctx *ctx = t->ctx;
    if (!q || !axes) return fail(ctx, WA_ERR_ARG, "%s: NULL axes or axes summary", who);
    if ((g == nullptr) != (tool == nullptr)) return fail(ctx, WA_ERR_ARG, "%s: a grid and a tool come together or not at all", who);
    if (g && g->ctx != ctx) return fail(ctx, WA_ERR_ARG, "%s: trajectory and grid belong to different contexts", who);
    const int64_t n = t->n;
    if (n < 2 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "%s: a trajectory needs 2 .. 2^31 samples", who);
    JerkAxesRun X;
    X.fr = fr;
    X.check = g != nullptr;
    X.axes_out = axes_out;
    X.blocked_out = blocked_out;
    X.out = axes;
    memset(&X.F, 0, sizeof X.F);
    if (tool && !torch_tool_dev(tool, near_add, &X.tool)) return fail(ctx, WA_ERR_ARG, "%s: n_beads, dist16, r2 or near_add out of range", who);
    if (!ax_pack(q, n, &X.hq)) return fail(ctx, WA_ERR_ARG, "%s: an axis component outside -16384 .. 16384 or an all-zero axis", who);
    if (g) {
        int rc = grid_field(g, &X.F);
        if (rc) return rc;
    }
    return jerk_run(who, g, t, lim, v_limit, dwell, tick, window, seg_tag, time_q_out, w_q_out, bound_out, ticks_out, s_q_out, tag_out, sum,
                    stops, jerk, &X);
}

int wa_traj_retime_jerk_axes(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, const double *dwell,
                             double tick, int32_t window, const uint8_t *seg_tag, const int32_t *q, const wa_tool_beads *tool,
                             int32_t near_add, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                             int64_t *s_q_out, uint8_t *tag_out, wa_traj **axes_out, uint8_t *blocked_out, wa_retime_summary *sum,
                             wa_stops_summary *stops, wa_jerk_summary *jerk, wa_jerk_axes_summary *axes)
{
    return jerk_axes_run("wa_traj_retime_jerk_axes", g, t, lim, v_limit, dwell, tick, window, seg_tag, q, tool, near_add, time_q_out, w_q_out,
                         bound_out, ticks_out, s_q_out, tag_out, axes_out, blocked_out, sum, stops, jerk, axes, nullptr);
}
