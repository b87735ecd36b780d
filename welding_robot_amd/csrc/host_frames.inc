// host_frames.inc -- C ABI: wa_traj_retime_jerk_frames, tool frames and the weld weave at jerk-limited ticks (included by weldacs.hip
// inside extern "C", behind host_jerk_axes.inc).  The call is wa_traj_retime_jerk_axes' body with one more policy in its tick kernel:
// the host checks the weave and turns the segment tags into the run bounds of rule 64 before anything is enqueued, jx_launch runs
// k_fr_dirs and k_fr_ticks in the place of k_jk_axes, and the frames record comes back with that call's records.
struct FramesRun {
    bool weave;                 // a wa_weave is given
    long long amp_q, wl_q, taper_q;
    int32_t P;
    std::vector<short> hpat;
    std::vector<int2> hrun;     // per segment: the samples O_r and E_r are taken at, x < 0 where it does not weave
    long long n_runs;
    wa_traj **lat_out;
    wa_frames_summary *out;
    WaFrRec rec;
    DevBuf<short4> tau;
    DevBuf<int2> run;
    DevBuf<short> pat;
    DevBuf<WaFrRec> drec;
    OwnedHandle<wa_traj> lat;
};

// rule 64 and the refusals of the frames section, from the arguments alone
static int fr_check(wa_ctx *ctx, const char *who, const wa_weave *w, const uint8_t *seg_tag, int64_t n, FramesRun *fr)
{
    fr->weave = w != nullptr;
    fr->n_runs = 0;
    if (!w) return WA_OK;
    if (!seg_tag) return fail(ctx, WA_ERR_ARG, "%s: a weave without seg_tag", who);
    if (!std::isfinite(w->amplitude) || w->amplitude < 0.0 || !std::isfinite(w->taper) || w->taper < 0.0 || !std::isfinite(w->wavelength))
        return fail(ctx, WA_ERR_ARG, "%s: amplitude and taper must be finite and >= 0, the wavelength finite", who);
    const double aq = rint(w->amplitude * WA_RT_Q), wq = rint(w->wavelength * WA_RT_Q), tq = rint(w->taper * WA_RT_Q);
    if (!(wq >= 1.0 && wq <= (double)WA_FR_MAX_WL)) return fail(ctx, WA_ERR_ARG, "%s: the wavelength must be 1 .. 2^50 quanta", who);
    if (!(aq < (double)WA_RT_CAP) || !(tq < (double)WA_RT_CAP)) return fail(ctx, WA_ERR_ARG, "%s: amplitude or taper reaches 2^61 quanta", who);
    if (w->P < 2 || w->P > WA_FR_MAX_P || !w->pattern) return fail(ctx, WA_ERR_ARG, "%s: a pattern needs 2 .. 4096 entries", who);
    if (w->pattern[0] != 0) return fail(ctx, WA_ERR_ARG, "%s: pattern[0] must be 0", who);
    for (int32_t j = 0; j < w->P; j++)
        if (w->pattern[j] < -16384 || w->pattern[j] > 16384) return fail(ctx, WA_ERR_ARG, "%s: a pattern entry outside -16384 .. 16384", who);
    if (w->tag_mask == 0) return fail(ctx, WA_ERR_ARG, "%s: tag_mask must not be 0", who);
    fr->amp_q = (long long)aq;
    fr->wl_q = (long long)wq;
    fr->taper_q = (long long)tq;
    fr->P = w->P;
    fr->hpat.assign(w->pattern, w->pattern + w->P);
    fr->hrun.assign((size_t)n - 1, make_int2(-1, -1));
    for (int64_t i = 0; i < n - 1;) {
        if ((seg_tag[i] & w->tag_mask) != w->tag_value) {
            i++;
            continue;
        }
        int64_t e = i;
        while (e + 1 < n - 1 && (seg_tag[e + 1] & w->tag_mask) == w->tag_value) e++;
        for (int64_t m = i; m <= e; m++) fr->hrun[(size_t)m] = make_int2((int)i, (int)(e + 1));   // (n <= 2^31: sample indices fit)
        fr->n_runs++;
        i = e + 1;
    }
    return WA_OK;
}

// behind k_jk_ticks in the place of k_jk_axes: A and the records are jx_launch's
static int fr_launch(wa_ctx *ctx, const WaJkTicks &T, long long n, const WaJkAxes &A, JerkRun &jk, FramesRun &Fr, const WaField &F,
                     const WaTorchTool *dtool, WaAxRec *drec)
{
    hipStream_t st = ctx->stream;
    const bool runs = Fr.weave && Fr.n_runs > 0;
    hipError_t e = Fr.tau.alloc((size_t)n);
    e = e ? e : Fr.drec.alloc(1);
    if (runs) {
        e = e ? e : Fr.run.alloc((size_t)n - 1);
        e = e ? e : Fr.pat.alloc((size_t)Fr.P);
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: device buffers of the frames", jk.who);
    wa_traj *l = nullptr;
    int rc = traj_alloc(ctx, T.n_ticks, &l);
    if (rc) return rc;
    Fr.lat.reset(l);
    e = hipMemsetAsync(Fr.drec, 0, sizeof(WaFrRec), st);
    if (runs) {
        e = e ? e : hipMemcpyAsync(Fr.run, Fr.hrun.data(), sizeof(int2) * ((size_t)n - 1), hipMemcpyHostToDevice, st);
        e = e ? e : hipMemcpyAsync(Fr.pat, Fr.hpat.data(), sizeof(short) * (size_t)Fr.P, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) {
        WaFrames W;
        W.tau = Fr.tau; W.run = runs ? Fr.run.p : nullptr; W.pat = Fr.pat; W.P = Fr.P; W.amp_q = Fr.amp_q; W.wl_q = Fr.wl_q;
        W.taper_q = Fr.taper_q; W.lat = Fr.lat->xyz; W.rec = Fr.drec;
        k_fr_dirs<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(T.xyz, T.GL, n, Fr.tau);
        k_fr_ticks<<<(unsigned)((T.n_ticks + 255) / 256), 256, 0, st>>>(T, A, F, dtool, drec, W);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", jk.who, hipGetErrorString(e));
    return WA_OK;
}

static hipError_t fr_copy_out(wa_ctx *ctx, FramesRun &Fr)
{
    if (!Fr.drec.p) return hipSuccess;
    return hipMemcpyAsync(&Fr.rec, Fr.drec, sizeof Fr.rec, hipMemcpyDeviceToHost, ctx->stream);
}

static void fr_summary(FramesRun &Fr, long long n_out, bool too_many)
{
    wa_frames_summary s;
    memset(&s, 0, sizeof s);
    if (!too_many) {
        s.n_ticks = n_out;
        for (int k = 0; k < WA_AX_SLOTS; k++) {
            s.n_no_lateral += (int64_t)Fr.rec.slot[k].n_no_lateral;
            s.n_weave_ticks += (int64_t)Fr.rec.slot[k].n_weave_ticks;
            s.n_weave_blocked += (int64_t)Fr.rec.slot[k].n_weave_blocked;
        }
        s.n_weave_runs = Fr.n_runs;
        s.max_offset_q = (int64_t)Fr.rec.max_offset_q;
        s.max_offset_step_q = (int64_t)Fr.rec.max_offset_step_q;
        s.max_lat_turn = (int64_t)Fr.rec.max_lat_turn;
    }
    if (Fr.lat_out) *Fr.lat_out = Fr.lat.release();   // (NULL above 2^31 ticks)
    *Fr.out = s;
}

int wa_traj_retime_jerk_frames(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, const double *dwell,
                               double tick, int32_t window, const uint8_t *seg_tag, const int32_t *q, const wa_tool_beads *tool,
                               int32_t near_add, const wa_weave *weave, int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out,
                               wa_traj **ticks_out, int64_t *s_q_out, uint8_t *tag_out, wa_traj **axes_out, uint8_t *blocked_out,
                               wa_traj **lat_out, wa_retime_summary *sum, wa_stops_summary *stops, wa_jerk_summary *jerk,
                               wa_jerk_axes_summary *axes, wa_frames_summary *frames)
{
    static const char *who = "wa_traj_retime_jerk_frames";
    if (!t) return WA_ERR_ARG;   // (nothing below touches the device before jerk_axes_run makes the context's device current)
    wa_ctx *ctx = t->ctx;
    if (!frames) return fail(ctx, WA_ERR_ARG, "%s: NULL frames summary", who);
    const int64_t n = t->n;
    if (n < 2 || n > WA_RT_MAX_N) return fail(ctx, WA_ERR_ARG, "%s: a trajectory needs 2 .. 2^31 samples", who);
    FramesRun Fr;
    Fr.lat_out = lat_out;
    Fr.out = frames;
    memset(&Fr.rec, 0, sizeof Fr.rec);
    int rc = fr_check(ctx, who, weave, seg_tag, n, &Fr);
    if (rc) return rc;
    return jerk_axes_run(who, g, t, lim, v_limit, dwell, tick, window, seg_tag, q, tool, near_add, time_q_out, w_q_out, bound_out, ticks_out,
                         s_q_out, tag_out, axes_out, blocked_out, sum, stops, jerk, axes, &Fr);
}
