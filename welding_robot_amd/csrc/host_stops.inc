// host_stops.inc -- C ABI: wa_traj_tick_axes_stops and wa_traj_axes_dwells, the weld passes in a timed trajectory (included by weldacs.hip
// inside extern "C"; wa_traj_retime_stops sits with the driver it shares, host_retime.inc).  As everywhere in the trajectory stages the
// host checks the arguments it is handed, the device the rest, and ONE record is read before any output is copied.
int wa_traj_tick_axes_stops(const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, int32_t near_add, double acc,
                            double dec, double tick, const int64_t *time_q, const int64_t *w_q, const uint8_t *seg_tag, wa_traj **axes_out,
                            uint8_t *blocked_out, uint8_t *tag_out, wa_tick_axes_summary *sum, wa_tick_stops_summary *stops)
{
    if (t && !stops) return fail(t->ctx, WA_ERR_ARG, "wa_traj_tick_axes_stops: NULL stops summary");
    if (t && tag_out && !seg_tag) return fail(t->ctx, WA_ERR_ARG, "wa_traj_tick_axes_stops: tag_out without seg_tag");
    return tick_axes_run("wa_traj_tick_axes_stops", g, t, q, tool, near_add, acc, dec, tick, time_q, w_q, seg_tag, axes_out, blocked_out,
                         tag_out, sum, stops);
}

int wa_traj_axes_dwells(const wa_traj *t, const int32_t *q, double omega, const double *dwell_in, double *dwell_out,
                        wa_axes_dwells_summary *sum)
{
    WaDevGuard dev_guard_(t ? t->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!t) return WA_ERR_ARG;
    wa_ctx *ctx = t->ctx;
    if (!q || !dwell_out || !sum) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: NULL argument");
    const int64_t n = t->n;
    if (n < 1 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: a trajectory needs 1 .. 2^31 samples");
    if (!rt_pos_finite(omega)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: omega must be finite and > 0");
    if (dwell_in)
        for (int64_t i = 0; i < n - 1; i++)
            if (!std::isfinite(dwell_in[i])) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: dwell_in entries must be finite");
    std::vector<short4> hq;
    if (!ax_pack(q, n, &hq)) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: an axis component outside -16384 .. 16384 or an all-zero axis");
    const size_t m = (size_t)n - 1;
    DevBuf<short4> dq;
    DevBuf<double> din, dout;
    DevBuf<WaDwRec> drec;
    hipError_t e = dq.alloc((size_t)n);
    e = e ? e : drec.alloc(1);
    if (m) e = e ? e : dout.alloc(m);
    if (m && dwell_in) e = e ? e : din.alloc(m);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_traj_axes_dwells: device buffers");
    hipStream_t st = ctx->stream;
    WaDwRec rec;
    e = hipMemcpyAsync(dq, hq.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
    e = e ? e : hipMemsetAsync(drec, 0, sizeof rec, st);
    if (m && dwell_in) e = e ? e : hipMemcpyAsync(din, dwell_in, sizeof(double) * m, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        k_ax_dwells<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t->xyz, dq, n, omega, din, dout, drec);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
    e = e ? e : hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_axes_dwells: %s", hipGetErrorString(e));
    if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: a coordinate of the trajectory is not finite");
    if (rec.bad & 8) return fail(ctx, WA_ERR_ARG, "wa_traj_axes_dwells: a dwell is given on a segment that has a length");
    // (every WA_ERR_ARG has been answered by now: nothing was written before this line)
    if (m) {
        e = hipMemcpyAsync(dwell_out, dout, sizeof(double) * m, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_axes_dwells: %s", hipGetErrorString(e));
    }
    wa_axes_dwells_summary s;
    memset(&s, 0, sizeof s);
    s.n = n;
    s.n_jump = (int64_t)rec.n_jump;
    s.n_stops = (int64_t)rec.n_stops;
    s.n_raised = (int64_t)rec.n_raised;
    memcpy(&s.max_need, &rec.max_need_bits, sizeof s.max_need);
    *sum = s;
    return WA_OK;
}
