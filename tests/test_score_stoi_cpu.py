"""STOI / ESTOI of the Scorer on the CPU (m2h/audio/score.py "STOI", tests/stoi_ref.py): properties of the definition in float64, the frame
counts and the band table, the NaN rules, the window-equals-slice construction, the float32 restatement that gives the GPU's end-to-end
tolerance, the mutant table, and the pure-Python plan of m2h.audio.score.

Measured here (float32 restatement against float64 over stoi_ref.cases()): worst |difference| of the six numbers 2.83e-8, so
TOL_END_TO_END = 2.3e-7; the mutants' smallest excess over that tolerance is printed by test_mutants_are_rejected."""
import numpy as np
import pytest

import stoi_ref as REF


def _one(L, seed=7, S=1, C=1, **kw):
    refs, est, mix, tg = REF.inputs(L, seed, S, C, **kw)
    return refs, est, mix, tg


def _x10(L=16000, seed=7):
    refs, est, mix, tg = _one(L, seed)
    return REF.resample(np.stack(REF.signals16(refs, est, mix, 0, tg)))


def test_band_table_matches_the_formula_bin_for_bin():
    assert [tuple(b) for b in REF.band_edges()] == list(zip(REF.EDGES[:-1], REF.EDGES[1:]))
    assert REF.EDGES[0] == 7 and REF.EDGES[-1] == 219 and len(REF.EDGES) == REF.BANDS + 1


def test_constants():
    assert REF.CLIP == 1.0 + 10.0 ** 0.75 and REF.EPS == np.finfo(np.float64).eps
    assert REF.W.shape == (256,) and np.array_equal(REF.W, np.hanning(258)[1:-1]) and REF.W[0] > 0


@pytest.mark.parametrize("L,frames,K", [(16000, 77, 61), (16001, 77, 61), (40001, 194, 154), (6000, 28, 20), (6560, 31, 23), (7000, 33, 25)])
def test_frame_counts_and_the_thirty_frame_rule(L, frames, K):
    refs, est, mix, tg = _one(L, 7 + L % 5)
    a = REF.analyse_recording(refs, est, mix, tg)
    whole = a["parts"][0][0]
    assert len(whole["mask"]) == frames == REF.frame_count(-(-L * 5 // 8)) and whole["K"] == K and whole["margin"] >= REF.MIN_MARGIN_DB
    assert whole["env"].shape == (3, 15, K - 1)
    assert np.isnan(a["six"][0, 0]).all() == (K - 1 < 30)
    if K - 1 >= 30:
        assert 0.98 < a["six"][0, 0, 0] < 1.0 and 0.9 < a["six"][0, 0, 1] < 1.0 and a["six"][0, 0, 4] > 0 and a["six"][0, 0, 5] > 0


def test_exclusive_end_drops_the_last_full_frame_and_an_input_without_gaps_keeps_all():
    L = REF.exclusive_end_length()
    n = -(-L * 5 // 8)
    assert (n - 256) % 128 == 0 and REF.frame_count(n) == (n - 256) // 128 == 80 and REF.frame_count(n + 1) == 81
    refs, est, mix, tg = _one(L, 7 + L % 5)
    assert len(REF.analyse_recording(refs, est, mix, tg)["parts"][0][0]["mask"]) == 80
    refs, est, mix, tg = _one(16000, 3, gaps=False)
    whole = REF.analyse_recording(refs, est, mix, tg)["parts"][0][0]
    assert whole["mask"].all() and whole["K"] == 77 and whole["margin"] >= REF.MIN_MARGIN_DB


def test_identity_scale_invariance_and_monotony():
    x10 = _x10()
    x = x10[0]
    a = REF.analyse(x, [x, 3.7 * x])
    assert abs(a["stoi"][0] - 1) <= 1e-12 and abs(a["estoi"][0] - 1) <= 1e-12 and abs(a["stoi"][1] - 1) <= 1e-12 and abs(a["estoi"][1] - 1) <= 1e-12
    y = x10[1]
    b = REF.analyse(x, [y, 0.01 * y, 250.0 * y])
    assert np.allclose(b["stoi"], b["stoi"][0], rtol=0, atol=1e-12) and np.allclose(b["estoi"], b["estoi"][0], rtol=0, atol=1e-12)
    noise = np.random.default_rng(5).standard_normal(len(x)) * 0.3
    c = REF.analyse(x, [x + g * noise for g in (0.1, 0.3, 1.0, 3.0)])
    assert all(np.diff(c["stoi"]) < 0) and all(np.diff(c["estoi"]) < 0), (c["stoi"], c["estoi"])


def test_nan_rules():
    x10 = _x10(7000, 9)
    a = REF.analyse(x10[0], [x10[1], x10[2]])
    assert a["K"] == 25 and np.isnan(REF.six(a)).all()
    z = np.zeros(10000)
    s = REF.analyse(z, [x10[1][:1] * z, z])
    assert s["silent"] and np.isnan(REF.six(s)).all()
    assert REF.analyse(z[:200], [z[:200], z[:200]])["K"] == 0 and np.isnan(REF.step3(np.ones((15, 29)), np.ones((15, 29)))).all()
    assert not np.isnan(REF.step3(np.random.default_rng(0).uniform(1, 2, (15, 30)), np.random.default_rng(1).uniform(1, 2, (15, 30)))).any()


@pytest.mark.parametrize("window,hop", [(1, 1), (2, 1)])
def test_a_window_is_the_whole_analysis_of_its_slice(window, hop):
    refs, est, mix, tg = _one(40001, 8, 3, 2)
    a = REF.analyse_recording(refs, est, mix, tg, window=window, hop=hop)
    assert a["ranges"][0] == (0, 25001) and a["ranges"][1:] == [(m * 10000, min((m + window) * 10000, 25001)) for m in range(len(a["ranges"]) - 1)]
    for c in range(2):
        for m, (s, e) in enumerate(a["ranges"][1:]):
            alone = REF.analyse(a["x10"][c, 0, s:e], [a["x10"][c, 1, s:e], a["x10"][c, 2, s:e]])
            assert np.array_equal(REF.six(alone), a["six"][c, 1 + m], equal_nan=True) and alone["K"] == a["K"][c, 1 + m]


def _worst(f32, defect=(), align=False):
    """the largest |restatement - float64| of the six numbers over stoi_ref.cases() (align: the aligned case alone)"""
    worst = 0.0
    if align:
        D, lags = 64, [37, 40]
        refs, _, mix, tg = REF.inputs(2 * D + 16001, 11, 3, 2)
        est = np.zeros_like(refs[0])
        for c in range(2):
            est[c, lags[c]:] = refs[tg, c, :refs.shape[-1] - lags[c]]
        est += (0.05 * np.random.default_rng(2).standard_normal(est.shape)).astype(np.float32)
        sets = [(refs, est, mix, tg, dict(lag=lags, D=D))]
    else:
        sets = [(refs, est, mix, tg, {}) for _, refs, est, mix, tg in REF.cases()]
    for refs, est, mix, tg, kw in sets:
        want = REF.analyse_recording(refs, est, mix, tg, **kw)["six"]
        got = REF.analyse_recording(refs, est, mix, tg, f32=f32, defect=defect, **kw)["six"]
        assert not np.isnan(want[:, 0]).any()
        d = np.abs(got - want)
        worst = max(worst, float(np.max(np.where(np.isnan(got) != np.isnan(want), np.inf, np.nan_to_num(d)))))
    return worst


def test_float32_restatement_gives_the_end_to_end_tolerance():
    worst = _worst(True)
    print("float32 restatement against float64: worst |difference| %.3e, 8 x = %.3e, TOL_END_TO_END = %.3e" % (worst, 8 * worst, REF.TOL_END_TO_END))
    assert 8 * worst <= REF.TOL_END_TO_END <= 1.25 * 8 * worst
    assert _worst(True, align=True) <= REF.TOL_END_TO_END / 8


def test_float32_restatement_keeps_the_mask_and_the_envelope_bound():
    """the element bound sqrt(bins) sqrt(2) TAU_FP32 |frame w| admits a correct float32 implementation, with the same kept frames"""
    worst = 0.0
    for _, refs, est, mix, tg in REF.cases():
        a, b = REF.analyse_recording(refs, est, mix, tg), REF.analyse_recording(refs, est, mix, tg, f32=True)
        for ra, rb in zip(a["parts"], b["parts"]):
            for pa, pb in zip(ra, rb):
                assert np.array_equal(pa["mask"], pb["mask"]) and pa["env"].shape == pb["env"].shape
                if pa["env"].size:
                    worst = max(worst, REF.worst(pb["env"], pa["env"], REF.env_bound(pa)))
    print("float32 restatement: envelopes worst error / bound %.3e" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("defect", REF.DEFECTS)
def test_mutants_are_rejected(defect):
    """every defect planted in the float32 restatement moves at least one of the six numbers of at least one input past the tolerance the
    GPU is held to; the correct restatement stays within it (the test above)"""
    worst = _worst(True, (defect,), align=defect == "no_lag")
    print("%-22s worst |difference| %.3e = %.0f x the tolerance" % (defect, worst, worst / REF.TOL_END_TO_END))
    assert worst > REF.TOL_END_TO_END


def test_step3_float64_against_longdouble():
    """the spread the GPU's segment kernel is held to, x 16 (tests/test_gpu_score_stoi.py measures it on the kernel's own envelopes)"""
    _, refs, est, mix, tg = REF.cases()[4]
    a = REF.analyse_recording(refs, est, mix, tg)["parts"][0][0]
    d64, dld = REF.step3(a["env"][0], a["env"][1]), REF.step3(a["env"][0], a["env"][1], dtype=np.longdouble)
    spread = max(abs(d64[0] - dld[0]), abs(d64[1] - dld[1]))
    print("step 3, float64 against longdouble: %.3e" % spread)
    assert spread < 1e-13


def test_plan_matches_the_reference_ranges():
    from m2h.audio import score as SC
    assert SC.STOI_ORDER == REF.ORDER
    assert np.array_equal(SC.stoi_window(), REF.W32)
    for L, D in ((6000, 0), (16000, 0), (16001, 0), (40001, 0), (16129, 64), (REF.exclusive_end_length(), 0)):
        for window, hop in ((1, 1), (2, 1), (1, 2)):
            plan = SC.score_plan(L, 16000, window, hop) if D == 0 else SC.align_plan(L, D, 16000, window, hop)
            sp = SC.stoi_plan(plan)
            if hop <= window:
                assert sp["ranges"] == REF.ranges(L - 2 * D, window, hop)
            frames = [SC.stoi_frames(e - s) for s, e in sp["ranges"]]
            assert frames == [REF.frame_count(e - s) for s, e in sp["ranges"]]
            ends = [s + f for s, f in zip(sp["slots"], frames)]
            assert sp["slots"][0] == 0 and all(a <= b for a, b in zip(ends, sp["slots"][1:] + [sp["total"]])) and sorted(sp["slots"]) == sp["slots"]
    with pytest.raises(ValueError, match="stoi=True needs tile = 16000 .*got 8000"):
        SC.stoi_plan(SC.score_plan(16000, 8000))
