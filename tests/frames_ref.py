"""numpy restatement of the tool frames and the weld weave at jerk-limited ticks (include/weldacs.h rules 61 - 67:
wa_traj_retime_jerk_frames), built on jerk_axes_ref (rules 56 - 60: S_k, the segment or stop of every filtered tick, its position, its
axis and the bead check).  What is stated here is the travel direction per sample (rule 62), the lateral per tick (rule 63), the runs
of weaving segments (rule 64), the offset (rule 65), the woven position with its check (rule 66) and the summary (rule 67): int64 and
individually rounded float64 operations.  No GPU, no product code.

A weave is dict(amplitude, wavelength, taper, pattern, tag_mask, tag_value)."""
import numpy as np

import jerk_axes_ref as X
import ticks_ref as K

T = K.T
Q = K.Q
QF = K.QF
CAP = K.CAP
MAX_P = 4096
MAX_WL = 1 << 50
FRAMES_FIELDS = ("n_ticks", "n_no_lateral", "n_weave_runs", "n_weave_ticks", "n_weave_blocked", "max_offset_q", "max_offset_step_q",
                 "max_lat_turn")


def weave(amplitude, wavelength, pattern, taper=0.0, tag_mask=0xff, tag_value=1):
    return dict(amplitude=amplitude, wavelength=wavelength, taper=taper, pattern=pattern, tag_mask=tag_mask, tag_value=tag_value)


def check_weave(w, seg_tag):
    """rule 61's refusals: (amp_q, wl_q, taper_q, pattern int64[P]); ValueError where the call answers WA_ERR_ARG"""
    if seg_tag is None:
        raise ValueError("a weave without seg_tag")
    a, l, t = (np.float64(w[k]) for k in ("amplitude", "wavelength", "taper"))
    if not (np.isfinite(a) and a >= 0 and np.isfinite(t) and t >= 0 and np.isfinite(l)):
        raise ValueError("amplitude, wavelength or taper")
    aq, lq, tq = np.rint(a * QF), np.rint(l * QF), np.rint(t * QF)
    if not 1 <= lq <= float(MAX_WL) or not aq < float(CAP) or not tq < float(CAP):
        raise ValueError("wl_q, amp_q or taper_q out of range")
    if w["pattern"] is None:
        raise ValueError("pattern")
    pat = np.asarray(w["pattern"], np.int64).reshape(-1)
    if not 2 <= len(pat) <= MAX_P or (np.abs(pat) > 16384).any() or pat[0] != 0 or not 1 <= int(w["tag_mask"]) <= 255:
        raise ValueError("pattern or tag_mask")
    return int(aq), int(lq), int(tq), pat


def directions(xyz, GL):
    """rule 62: tau int64[n, 3], (0, 0, 0) where the direction is all zero"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(GL)
    j = np.arange(n)
    lo = np.searchsorted(GL, GL, side="left") - 1    # GL never falls: the highest m < j with GL_m < GL_j
    hi = np.searchsorted(GL, GL, side="right")       # the lowest m > j with GL_m > GL_j
    a, b = p[np.where(lo >= 0, lo, j)], p[np.where(hi < n, hi, j)]
    Tj = b - a
    tau = np.zeros((n, 3), np.int64)
    nz = ~(Tj == 0).all(1)
    if nz.any():
        tau[nz] = K.quantise_rows(Tj[nz])
    return tau


def laterals(r, tau):
    """rule 63 on jerk_axes_ref's dictionary: (ql int64[n_ticks, 3], t int64[n_ticks, 3]); ql all zero where it is undefined"""
    seg, rest, lam, qt, GL = r["seg"], r["rest"], r["lam"], r["qt"], r["GL"]
    a, _ = X.runs(GL, seg)
    t, _ = X.interpolate(tau[seg], tau[seg + 1], lam)
    t[rest] = tau[a[rest]]
    z = qt.astype(np.float64)
    u = t.astype(np.float64)
    y = np.stack([z[:, 1] * u[:, 2] - z[:, 2] * u[:, 1], z[:, 2] * u[:, 0] - z[:, 0] * u[:, 2], z[:, 0] * u[:, 1] - z[:, 1] * u[:, 0]], 1)
    ql = np.zeros_like(qt)
    nz = ~(y == 0).all(1)
    if nz.any():
        ql[nz] = K.quantise_rows(y[nz])
    return ql, t


def run_bounds(seg_tag, mask, value):
    """rule 64: (weaves bool[n-1], lo int64[n-1], hi int64[n-1], n_runs); lo and hi mean nothing where a segment does not weave"""
    wv = (np.asarray(seg_tag, np.uint8) & np.uint8(mask)) == np.uint8(value)
    m = len(wv)
    lo, hi = np.zeros(m, np.int64), np.zeros(m, np.int64)
    begins = np.flatnonzero(wv & ~np.concatenate([[False], wv[:-1]]))
    ends = np.flatnonzero(wv & ~np.concatenate([wv[1:], [False]]))
    for b, e in zip(begins, ends):
        lo[b:e + 1], hi[b:e + 1] = b, e
    return wv, lo, hi, len(begins)


def offsets(S_q, seg, GL, wv, lo, hi, amp_q, wl_q, taper_q, pat):
    """rule 65: (off float64[n_ticks], off_q int64[n_ticks], weaving mask)"""
    P = len(pat)
    on = wv[seg]
    d = np.where(on, S_q - GL[lo[seg]], 0)
    back = np.where(on, GL[hi[seg] + 1] - S_q, 0)
    phi = d % wl_q
    x = (phi.astype(np.float64) * np.float64(P)) / np.float64(wl_q)
    j = np.minimum(np.floor(x).astype(np.int64), P - 1)
    f = x - j.astype(np.float64)
    pa, pb = pat[j].astype(np.float64), pat[(j + 1) % P].astype(np.float64)
    w = pa + (pb - pa) * f
    m = np.minimum(d, back)
    with np.errstate(divide="ignore", invalid="ignore"):
        env = np.where((taper_q == 0) | (m >= taper_q), 1.0, m.astype(np.float64) / np.float64(taper_q))
    off = (((np.float64(amp_q) / QF) * env) * w) / 16384.0
    off = np.where(on, off, 0.0)
    return off, np.rint(off * QF).astype(np.int64), on


def weave_positions(ticks, ql, off):
    """rule 66: the woven positions float32[n_ticks, 3] and the mask of the ticks that moved"""
    moved = (off != 0) & (ql != 0).any(1)
    out = np.asarray(ticks, np.float32).copy()
    out[moved] = (out[moved].astype(np.float64) + (ql[moved].astype(np.float64) / 16384.0) * off[moved, None]).astype(np.float32)
    return out, moved


def retime_jerk_frames(xyz, q, lim, dwell=None, window=1, v_limit=None, grid=None, tool=None, near_add=-1, tick=0.01, seg_tag=None,
                       weave=None):
    """wa_traj_retime_jerk_frames: jerk_axes_ref.retime_jerk_axes' dictionary with the woven `ticks`, the woven `blocked` and the axes
    summary that goes with them, plus lat float32[n_ticks, 3], ql, off, off_q, weaving, moved, tau, frames_summary and base_ticks (rule
    54's positions); ValueError where the call answers WA_ERR_ARG.  Above 2^31 ticks lat is None and the frames summary all zero."""
    par = check_weave(weave, seg_tag) if weave is not None else None
    r = X.retime_jerk_axes(xyz, q, lim, dwell, window, v_limit, grid, tool, near_add, tick, seg_tag)
    if r["s_q"] is None:
        return dict(r, lat=None, frames_summary=dict.fromkeys(FRAMES_FIELDS, 0))
    GL, seg, S_q = r["GL"], r["seg"], r["s_q"]
    m = len(S_q)
    tau = directions(xyz, GL)
    ql, t = laterals(r, tau)
    off, off_q, on, n_runs = np.zeros(m), np.zeros(m, np.int64), np.zeros(m, bool), 0
    if par is not None:
        wv, lo, hi, n_runs = run_bounds(seg_tag, weave["tag_mask"], weave["tag_value"])
        off, off_q, on = offsets(S_q, seg, GL, wv, lo, hi, *par)
    ticks, moved = weave_positions(r["ticks"], ql, off)
    out = dict(r, base_ticks=r["ticks"], ticks=ticks)
    blocked = r["blocked"].astype(bool)
    if grid is not None and moved.any():   # rule 66: rule 59 at the woven positions
        vox, outside = T.sample_voxels(grid, ticks)
        blocked, near = K.blocked_at(grid, vox, r["qt"], tool, near_add)
        out["axes_summary"] = dict(r["axes_summary"], n_outside=int(outside.sum()), n_blocked=int(blocked.sum()),
                                   first_blocked=int(np.flatnonzero(blocked)[0]) if blocked.any() else -1,
                                   n_near=int((~blocked & (near > 0)).sum()))
        out["blocked"] = blocked.astype(np.uint8)
    has = (ql != 0).any(1)
    both = has[1:] & has[:-1]
    lt = T.turn(ql[:-1], ql[1:])[both]
    step = np.abs(np.diff(off_q))
    summary = dict(n_ticks=m, n_no_lateral=int((~has).sum()), n_weave_runs=int(n_runs), n_weave_ticks=int(on.sum()),
                   n_weave_blocked=int((on & blocked).sum()), max_offset_q=int(np.abs(off_q).max()),
                   max_offset_step_q=int(step.max()) if len(step) else 0, max_lat_turn=int(lt.max()) if len(lt) else 0)
    out.update(lat=(ql.astype(np.float64) / 16384.0).astype(np.float32), ql=ql, t=t, tau=tau, off=off, off_q=off_q, weaving=on, moved=moved,
               frames_summary=summary)
    return out


def frames_scalar(r, xyz, seg_tag=None, weave=None):
    """rules 62 - 66 once more on the located ticks of r (jerk_axes_ref's dictionary: seg, rest, lam, qt, s_q, GL, base_ticks), one tick after
    the other with Python integers and numpy float64 scalars: (ql list of triples, off_q list, positions float32[n_ticks, 3])"""
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    GL = [int(g) for g in r["GL"]]
    n = len(GL)
    f64 = np.float64

    def rule1(v):
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return [int(np.rint((c / ln) * f64(16384.0))) for c in v]

    tau = []
    for j in range(n):
        lo = max([m for m in range(j) if GL[m] < GL[j]], default=None)
        hi = min([m for m in range(j + 1, n) if GL[m] > GL[j]], default=None)
        a, b = p32[j if lo is None else lo], p32[j if hi is None else hi]
        v = [f64(b[c]) - f64(a[c]) for c in range(3)]
        tau.append([0, 0, 0] if all(c == 0 for c in v) else rule1(v))
    if weave is not None:
        amp_q, wl_q, taper_q, pat = check_weave(weave, seg_tag)
        pat = [int(c) for c in pat]
        P = len(pat)
        on = [(int(s) & int(weave["tag_mask"])) == int(weave["tag_value"]) for s in np.asarray(seg_tag).reshape(-1)]
    qls, offs, pos = [], [], np.asarray(r["base_ticks"], np.float32).copy()
    for k in range(len(r["s_q"])):
        i, S, lam = int(r["seg"][k]), int(r["s_q"][k]), f64(r["lam"][k])
        if r["rest"][k]:
            t = tau[min(m for m in range(n) if GL[m] == GL[i])]
        else:
            v = [f64(tau[i][c]) + (f64(tau[i + 1][c]) - f64(tau[i][c])) * lam for c in range(3)]
            t = list(tau[i]) if all(c == 0 for c in v) else rule1(v)
        z = [int(c) for c in r["qt"][k]]
        y = [z[1] * t[2] - z[2] * t[1], z[2] * t[0] - z[0] * t[2], z[0] * t[1] - z[1] * t[0]]
        ql = [0, 0, 0] if not any(y) else rule1([f64(c) for c in y])
        off = f64(0.0)
        if weave is not None and on[i]:
            lo = i
            while lo > 0 and on[lo - 1]:
                lo -= 1
            hi = i
            while hi + 1 < n - 1 and on[hi + 1]:
                hi += 1
            d, back = S - GL[lo], GL[hi + 1] - S
            x = (f64(d % wl_q) * f64(P)) / f64(wl_q)
            j = min(int(np.floor(x)), P - 1)
            w = f64(pat[j]) + (f64(pat[(j + 1) % P]) - f64(pat[j])) * (x - f64(j))
            m = min(d, back)
            env = f64(1.0) if taper_q == 0 or m >= taper_q else f64(m) / f64(taper_q)
            off = (((f64(amp_q) / QF) * env) * w) / f64(16384.0)
        qls.append(ql)
        offs.append(int(np.rint(off * QF)))
        if off != 0 and any(ql):
            pos[k] = [np.float32(f64(pos[k][c]) + (f64(ql[c]) / f64(16384.0)) * off) for c in range(3)]
    return qls, offs, pos


# ------------------------------------------------------------------ scenes for the tests
def triangle(P):
    """a triangle wave as an int16-ranged table of P entries: 0, up to +16384 at a quarter, down to -16384 at three quarters"""
    u = np.arange(P, dtype=np.float64) / P
    tri = np.where(u < 0.25, 4.0 * u, np.where(u < 0.75, 2.0 - 4.0 * u, 4.0 * u - 4.0))
    out = np.rint(tri * 16384.0).astype(np.int64)
    out[0] = 0
    return out


def snap(x):
    """the nearest multiple of 2^-30: rint(x * Q) / Q is then x itself"""
    return float(np.rint(np.float64(x) * QF) / QF)


def random_case(seed):
    """jerk_axes_ref.random_case(seed) with tags that put one to three weld passes on the path (tag 1 on a stretch of segments, stops
    inside included, 0 elsewhere; every third case has bit 1 set elsewhere to exercise the mask) and a weave: amplitude 0.05 .. 0.6,
    wavelength 0.2 .. 3, taper 0, short, or longer than the runs, a triangle or random pattern of 2 .. 33 entries.  Every seventh case has
    no weave."""
    c = X.random_case(seed)
    rs = np.random.RandomState(7000 + seed)
    n = len(c["xyz"])
    tag = np.zeros(n - 1, np.uint8)
    for _ in range(int(rs.randint(1, 4))):
        a = int(rs.randint(0, n - 1))
        tag[a:a + int(rs.randint(1, max(2, n // 2)))] = 1
    if seed % 3 == 0:
        tag |= (rs.randint(0, 2, n - 1) * 2).astype(np.uint8)
    P = int(rs.choice([2, 3, 8, 33]))
    pat = triangle(P) if rs.uniform() < 0.5 else np.concatenate([[0], rs.randint(-16384, 16385, P - 1)]).astype(np.int64)
    wv = weave(snap(rs.uniform(0.05, 0.6)), snap(rs.uniform(0.2, 3.0)), pat, snap(rs.choice([0.0, 0.3, 50.0])), 1, 1)
    return dict(c, tag=tag, weave=None if seed % 7 == 6 else wv)
