"""The rules of the tool frames and the weld weave at jerk-limited ticks (include/weldacs.h rules 61 - 67), held against themselves on the
CPU: the array form of tests/frames_ref.py against a per-tick loop, the bytes that stay without a weave, and the properties the rules
promise.  No GPU, no product code."""
import numpy as np
import pytest

import frames_ref as F
import jerk_axes_ref as X

SEEDS = list(range(40))


def run(c, window, weave="case", **kw):
    a = dict(dwell=c["dwell"], window=window, grid=c["grid"], tool=c["tool"], near_add=c["near_add"], tick=c["tick"], seg_tag=c["tag"])
    a.update(kw)
    return F.retime_jerk_frames(c["xyz"], c["q"], c["lim"], weave=c["weave"] if weave == "case" else weave, **a)


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed in SEEDS:
        c = F.random_case(seed)
        W = [1, 2, 5, 17][seed % 4]
        out.append((c, W, run(c, W)))
    return out


def test_array_form_against_a_per_tick_loop(cases):
    woven = 0
    for c, W, r in cases:
        ql, off_q, pos = F.frames_scalar(r, c["xyz"], c["tag"], c["weave"])
        assert np.array_equal(np.asarray(ql, np.int64).reshape(-1, 3), r["ql"])
        assert np.array_equal(np.asarray(off_q, np.int64), r["off_q"])
        assert pos.tobytes() == r["ticks"].tobytes()
        woven += int(r["moved"].sum())
    assert woven > 1000   # (the cases do weave)


def test_without_a_weave_every_shared_output_is_jerk_axes_ref(cases):
    for c, W, _ in cases[::3]:
        base = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c["dwell"], W, None, c["grid"], c["tool"], c["near_add"], c["tick"], c["tag"])
        for weave in (None, dict(c["weave"] or F.weave(0.25, 1.0, F.triangle(8)), amplitude=0.0),
                      dict(c["weave"] or F.weave(0.25, 1.0, F.triangle(8)), tag_mask=0x80, tag_value=0x80)):
            r = run(c, W, weave)
            for k in ("time_q", "w_q", "bound", "ticks", "s_q", "tag", "axes", "blocked"):
                assert np.asarray(r[k]).tobytes() == np.asarray(base[k]).tobytes(), k
            for k in ("summary", "stops", "jerk", "axes_summary"):
                assert r[k] == base[k], k
            assert r["frames_summary"]["max_offset_q"] == 0 and not r["moved"].any()


def test_a_weave_changes_only_what_rule_61_lets_it_change(cases):
    for c, W, r in cases:
        base = X.retime_jerk_axes(c["xyz"], c["q"], c["lim"], c["dwell"], W, None, c["grid"], c["tool"], c["near_add"], c["tick"], c["tag"])
        for k in ("time_q", "w_q", "bound", "s_q", "tag", "axes"):
            assert np.asarray(r[k]).tobytes() == np.asarray(base[k]).tobytes(), k
        for k in ("summary", "stops", "jerk"):
            assert r[k] == base[k], k
        for k in ("n_ticks", "max_tick_turn", "n_rest_ticks", "n_turning_rests", "min_turn_ticks", "max_rest_turn"):
            assert r["axes_summary"][k] == base["axes_summary"][k], k
        assert np.array_equal(r["ticks"][~r["moved"]], base["ticks"][~r["moved"]])


def test_offset_stays_within_the_amplitude(cases):
    for c, W, r in cases:
        if c["weave"] is None:
            continue
        amp = c["weave"]["amplitude"]   # (a multiple of 2^-30: amp_q / Q is the amplitude itself)
        assert np.rint(np.float64(amp) * F.QF) / F.QF == amp
        assert (np.abs(r["off"]) <= amp).all() and r["frames_summary"]["max_offset_q"] <= int(np.rint(amp * F.QF))
        assert (r["off"][~r["weaving"]] == 0).all()


def test_offset_is_zero_at_both_ends_of_a_run_with_a_taper(cases):
    seen = 0
    for c, W, r in cases:
        if c["weave"] is None or c["weave"]["taper"] == 0:
            continue
        par = F.check_weave(c["weave"], c["tag"])
        wv, lo, hi, n_runs = F.run_bounds(c["tag"], c["weave"]["tag_mask"], c["weave"]["tag_value"])
        segs = np.flatnonzero(wv)
        GL = r["GL"]
        at_O, _, on = F.offsets(GL[lo[segs]], lo[segs], GL, wv, lo, hi, *par)
        at_E, _, _ = F.offsets(GL[hi[segs] + 1], hi[segs], GL, wv, lo, hi, *par)
        assert on.all() and (at_O == 0).all() and (at_E == 0).all()
        seen += n_runs
    assert seen > 10


def test_lateral_is_orthogonal_to_the_axis_within_the_derived_bound(cases):
    """y = qt x t is formed in exact integers, so y . qt = 0 exactly.  Rule 1 gives ql_c = 16384 * y_c / |y| + e_c with |e_c| <= 1/2 from the
    rint plus what two double operations (a division and a product, each within 2^-53 relative) add to a value of at most 16384:
    below 2^-38.  So |ql . qt| = |e . qt| <= |e| * |qt| with |e| <= sqrt(3) * (1/2 + 2^-38), and qt, itself a rule-1 triple, has
    |qt| <= 16384 + sqrt(3) / 2."""
    bound = (np.sqrt(3.0) * (0.5 + 2.0 ** -38)) * (16384.0 + np.sqrt(3.0) / 2.0) / 2.0 ** 28
    worst = 0.0
    for c, W, r in cases:
        assert r["frames_summary"]["n_no_lateral"] == 0   # (what follows relies on a defined lateral)
        dot = np.abs((r["ql"] * r["qt"]).sum(1)) / 2.0 ** 28
        worst = max(worst, float(dot.max()))
        assert (dot <= bound).all()
        ln = np.sqrt((r["ql"].astype(np.float64) ** 2).sum(1))
        assert (np.abs(ln - 16384.0) <= np.sqrt(3.0) / 2.0 + 1e-6).all()
    assert 0 < worst <= bound < 6e-5


def rest_in_a_run():
    """a pass along +x with a stop of 0.2 s in its middle, over which the torch turns from (0, -1, 1) to (0, 1, 1); every segment weaves"""
    xyz, dwell = X.polyline([([[2, 8, 8], [5, 8, 8], [8, 8, 8]], []), ([[8, 8, 8], [11, 8, 8], [14, 8, 8]], [0.2])])
    n = len(xyz)
    q = np.tile(X.fixed_axis((0.0, -1.0, 1.0)), (n, 1))
    q[3:] = X.fixed_axis((0.0, 1.0, 1.0))
    import retime_ref as R
    lim = R.limits(v_max=6.0, acc=12.0, dec=12.0, a_lat=10.0, v_near=2.0, near_d2=2)
    return dict(xyz=xyz, dwell=dwell, q=q, lim=lim, tag=np.ones(n - 1, np.uint8), weave=F.weave(0.25, 1.625, F.triangle(16), 0.5))


def test_a_rest_inside_a_run_keeps_its_offset_while_the_lateral_turns():
    c = rest_in_a_run()
    r = F.retime_jerk_frames(c["xyz"], c["q"], c["lim"], c["dwell"], 4, seg_tag=c["tag"], weave=c["weave"])
    rest = np.flatnonzero(r["rest"])
    assert len(rest) >= 20 and r["frames_summary"]["n_weave_runs"] == 1 and r["weaving"].all() and r["frames_summary"]["n_no_lateral"] == 0
    assert len(set(r["off_q"][rest].tolist())) == 1 and r["off_q"][rest[0]] != 0
    assert not np.array_equal(r["ql"][rest[0]], r["ql"][rest[-1]]) and len({tuple(v) for v in r["ql"][rest].tolist()}) > 10
    assert r["moved"][rest].all() and len({tuple(v) for v in r["ticks"][rest].tolist()}) > 10   # (the tip swings with the lateral)


def test_sign_of_the_lateral():
    """torch body up, travel along +x: the lateral is +y"""
    c = rest_in_a_run()
    q = np.tile(np.array([0, 0, 16384]), (len(c["xyz"]), 1))
    r = F.retime_jerk_frames(c["xyz"], q, c["lim"], c["dwell"], 1)
    assert (r["ql"] == np.array([0, 16384, 0])).all() and (r["tau"] == np.array([16384, 0, 0])).all()


@pytest.mark.parametrize("change", [dict(amplitude=-0.1), dict(amplitude=float("inf")), dict(taper=float("nan")), dict(taper=-1.0),
                                    dict(wavelength=float("inf")), dict(wavelength=0.0), dict(wavelength=-1.0), dict(wavelength=2.0 ** 21),
                                    dict(amplitude=2.0 ** 31), dict(taper=2.0 ** 31), dict(pattern=[0]), dict(pattern=[0] * 4097),
                                    dict(pattern=None), dict(pattern=[0, 16385]), dict(pattern=[0, -16385]), dict(pattern=[1, 0]),
                                    dict(tag_mask=0)])
def test_refusals(change):
    c = rest_in_a_run()
    with pytest.raises(ValueError):
        F.retime_jerk_frames(c["xyz"], c["q"], c["lim"], c["dwell"], 2, seg_tag=c["tag"], weave=dict(c["weave"], **change))


def test_a_weave_needs_tags():
    c = rest_in_a_run()
    with pytest.raises(ValueError):
        F.retime_jerk_frames(c["xyz"], c["q"], c["lim"], c["dwell"], 2, weave=c["weave"])
