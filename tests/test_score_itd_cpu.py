"""The Scorer's broadband ITD without a GPU: itd_table(), the pick and the nine numbers of itd_from_gcc, the bound of tests/itd_ref.py (it
admits a correct fp32 implementation and rejects the defects a fused GCC-PHAT can have), the margins of every case the GPU test uses,
and the refusals of m2h_score_itd, m2h_itd_gcc and Scorer.score(itd=True).

Measured (E, margins, worst error / bound, misses of the planted defects): DESIGN.md §8.12."""
import ctypes

import numpy as np
import pytest
import torch

import itd_ref as REF
import spatial_ref as PR
from m2h import _lib
from m2h.audio import score as SC

_cases = {}
# what G of one coherent source (a peak of 1) loses one grid step from its peak, 6.4e-3: a bound E below half of it resolves such a peak
UNIT_DROP = float(np.mean(1.0 - np.cos(2.0 * np.pi * np.arange(*REF.BINS) / (1023.0 * REF.UPSAMPLE))))


def case(name):
    """-> (sig: the three binaural signals as float64 rows, sums [3, 256, 2], bound [3, 256]) of tile 0; made once, shared and read-only"""
    if name not in _cases:
        refs, est, mix = PR.click_pairs() if name == "clicks" else PR.binaural() if name == "binaural" else REF.planted(name, REF.TILE)
        sig = REF.signals(refs, est, mix)
        sums, bound = REF.tile_sums(sig, 0)
        for a in [x for pair in sig for x in pair] + [sums, bound]:
            a.setflags(write=False)
        _cases[name] = (sig, sums, bound)
    return _cases[name]


def test_constants_and_table():
    assert tuple(SC.ITD_ORDER) == REF.ORDER and tuple(SC.ITD_BINS) == REF.BINS == (6, 256) and SC.ITD_MAX_LAG == 16 and SC.ITD_UPSAMPLE == 8
    assert SC.ITD_LAGS == REF.NL == 257 and SC.ITD_US_PER_STEP == REF.US_PER_STEP == 7.8125
    t = SC.itd_table()
    q = np.arange(8184, dtype=np.float64)
    assert t.dtype == np.float64 and t.shape == (8184, 2) and t.flags["C_CONTIGUOUS"]
    d = max(np.abs(t[:, 0] - np.cos(2.0 * np.pi * q / 8184.0)).max(), np.abs(t[:, 1] - np.sin(2.0 * np.pi * q / 8184.0)).max())
    print("itd_table against float64 cos and sin: %.3e" % d)
    assert d <= 4 * np.finfo(np.float64).eps                                             # (the angle itself is rounded: 2 pi q / 8184 <= 2 pi)
    assert t[0].tolist() == [1.0, 0.0] and t[4092, 0] == -1.0 and abs(t[2046, 1] - 1.0) <= 1e-16


def test_pick_ties_go_to_the_smallest_lag_then_the_negative_one():
    g = np.zeros((6, 3, 257))
    g[1, :, [128 + 9, 128 - 9]] = 0.5                                                    # equal maxima at -9 and +9: the negative one
    g[2, :, [128 + 9, 128 - 4]] = 0.5                                                    # at -4 and +9: the smaller |i|
    g[3, :, [128 + 3, 128 - 9]] = 0.5                                                    # at +3 and -9: the smaller |i|
    g[4] = -1.0                                                                          # G itself, not |G|: the least negative
    g[4, :, 128 + 77] = -0.25
    g[5, :, [0, 256]] = 0.5                                                              # both edges
    got = SC.itd_from_gcc(torch.from_numpy(g))
    assert got.dtype == torch.float64 and tuple(got.shape) == (6, 9)
    want = np.array([0.0, -9.0, -4.0, 3.0, 77.0, -128.0]) * 7.8125
    assert (got[:, 0].numpy() == want).all() and (got[:, 1].numpy() == want).all() and (got[:, 2].numpy() == want).all()
    assert got[:, 6].tolist() == [0.0, 0.5, 0.5, 0.5, -0.25, 0.5]
    assert (got[:, 3:6].numpy() == 0).all()                                              # an all-zero row picks lag 0 and peak 0: no NaN without `has`
    assert (REF.nine(g)[:, :3] == got[:, :3].numpy()).all()
    # a signal without a bin in the band: itd and peak NaN, and what follows from them
    has = torch.tensor([[True, True, True], [False, True, True], [True, False, True], [True, True, False]])
    got = SC.itd_from_gcc(torch.from_numpy(g[:4]), has).numpy()
    nan = np.isnan(got)
    assert not nan[0].any()
    assert nan[1].tolist() == [True, False, False, True, True, True, True, False, False]   # a silent target: itd, itd_err, itd_err_base, itd_erri, peak
    assert nan[2].tolist() == [False, True, False, True, False, True, False, True, False]
    assert nan[3].tolist() == [False, False, True, False, True, True, False, False, True]
    with pytest.raises(TypeError, match="float64"):
        SC.itd_from_gcc(torch.zeros(3, 257))
    with pytest.raises(ValueError, match=r"\[3, 257\]"):
        SC.itd_from_gcc(torch.zeros(3, 256, dtype=torch.float64))


def test_sign_convention_a_late_right_ear_is_a_positive_itd():
    r = np.random.default_rng(4)
    x = r.standard_normal(REF.TILE + 5)
    g = np.stack([x[5:], x[:-5]])                                                        # right[t] = left[t - 5]
    sums = REF.tile_sums(((g[0], g[1]), (g[1], g[0]), (g[0], g[0])), 0)[0]              # the estimate: the ears swapped; the mixture: no delay
    got = SC.itd_from_gcc(torch.from_numpy(REF.gcc(sums)), SC.itd_has_band(torch.from_numpy(sums))).numpy()
    print("ITD of a right ear 5 samples late: %s" % got)
    assert got[:3].tolist() == [312.5, -312.5, 0.0] and got[3:6].tolist() == [625.0, 312.5, -312.5] and (got[6:] > 0.99).all()


def test_the_nine_numbers_against_the_reference_algebra():
    r = np.random.default_rng(1)
    g = r.uniform(-1.0, 1.0, (2, 5, 3, 257))
    sums = r.standard_normal((2, 5, 3, 256, 2))
    sums[0, 1, 0] = 0.0                                                                  # a silent target
    sums[1, 2, 1, 6:] = 0.0                                                              # an estimate with energy below the band only
    sums[1, 3, 2, :255] = 0.0                                                            # a mixture with its last bin only: it has a band
    has = SC.itd_has_band(torch.from_numpy(sums))
    assert (has.numpy() == REF.has_band(sums)).all() and int((~has).sum()) == 2 and not has[0, 1, 0] and not has[1, 2, 1]
    got, want = SC.itd_from_gcc(torch.from_numpy(g), has).numpy(), REF.nine(g, REF.has_band(sums))
    assert (np.isnan(got) == np.isnan(want)).all() and np.isnan(want).sum() == 5 + 4
    assert (got[~np.isnan(want)] == want[~np.isnan(want)]).all()                         # grid values and copies of G: exact


@pytest.mark.parametrize("name", [0, 1, "clicks", "binaural"])
def test_float32_restatement_stays_within_the_bound(name):
    sig, want, bound = case(name)
    got = REF.tile_sums32(sig, 0)
    w = REF.worst(got, want, bound[..., None])
    g64, g32, E = REF.gcc(want), REF.gcc(got), REF.gcc_bound(want, bound)
    wg = float((np.abs(g32 - g64) / E[:, None]).max())
    _, _, margin = REF.pick(g64)
    print("float32 restatement, %s: Phi worst error / bound %.3e; G worst error %.3e, worst error / E %.3e; E %s; margin %s; margin / 2E %s"
          % (name, w, np.abs(g32 - g64).max(), wg, E, margin, margin / (2 * E)))
    assert want.shape == (3, 256, 2) and g64.shape == (3, 257) and w <= 1.0 and wg <= 1.0
    assert (E < 0.5 * UNIT_DROP).all() and (REF.pick(g32)[0] == REF.pick(g64)[0]).all()


def _misses(got, want, tol):
    return np.abs(got - want) / tol


SUM_DEFECTS = {"the conjugate on the wrong factor": dict(wrong_conj=True), "ears swapped": dict(swap_ears=True)}
GCC_DEFECTS = {"the band starts one bin early": dict(bins=(5, 256)), "the band starts one bin late": dict(bins=(7, 256)),
               "the band ends one bin early": dict(bins=(6, 255)), "PHAT left out": dict(phat=False), "a twiddle for U = 16": dict(upsample=16),
               "the lag's sign flipped": dict(flip=True)}


@pytest.mark.parametrize("defect", sorted(SUM_DEFECTS))
def test_the_bound_rejects_the_defect_in_the_sums(defect):
    sig, want, bound = case("binaural")
    assert REF.worst(REF.tile_sums32(sig, 0), want, bound[..., None]) <= 1.0
    miss = _misses(REF.tile_sums32(sig, 0, **SUM_DEFECTS[defect]), want, bound[..., None])
    print("%s: %d of %d sums missed, the largest by %.2g bounds" % (defect, int((miss > 1.0).sum()), miss.size, miss.max()))
    assert miss.max() > 1.0


def _tones():
    """the binaural noise case plus tone pairs at the bins 5 / 6 and 255 / 256, each tone with a delay of its own: tile sums [3, 256, 2], bound"""
    if "tones" not in _cases:
        refs, est, mix = (np.asarray(a, np.float64) for a in PR.binaural(seed=5))
        tones = 0.05 * (REF.tone_pair(5, 6, -6, 7) + REF.tone_pair(255, 256, 3, -2))
        _cases["tones"] = REF.tile_sums(REF.signals(refs + tones, est + tones, mix + tones), 0)
    return _cases["tones"]


@pytest.mark.parametrize("defect", sorted(GCC_DEFECTS))
def test_the_bound_rejects_the_defect_in_the_function(defect):
    for name, (want, bound) in (("binaural", case("binaural")[1:]), ("tones", _tones())):
        g, E = REF.gcc(want), REF.gcc_bound(want, bound)
        miss = _misses(REF.gcc(want, **GCC_DEFECTS[defect]), g, E[:, None])
        print("%s, %s: %d of %d values of G missed, the largest by %.2g E (E %s)" % (defect, name, int((miss > 1.0).sum()), miss.size, miss.max(), E))
        assert (E < 0.5 * UNIT_DROP).all() and miss.max() > 1.0


def test_the_bound_rejects_the_right_ear_read_at_a_lag_of_its_own():
    """D = 64: the estimate's ears are the target's, late by 37 and 40 samples.  At ONE lag the 3 samples of interaural delay the estimate
    added are measured; with each ear at its own lag they are cancelled."""
    D, lags, L = 64, (37, 40), 2 * 64 + 16000
    r = np.random.default_rng(11)
    refs = (0.1 * r.standard_normal((1, 2, L))).astype(np.float32)
    refs[0, 1, 5:] = refs[0, 0, :L - 5]                                                  # the target: 5 samples
    est = np.zeros((2, L), np.float32)
    for c in range(2):
        est[c, lags[c]:] = refs[0, c, :L - lags[c]]
    est += (0.001 * r.standard_normal(est.shape)).astype(np.float32)
    mix = (refs[0] + 0.05 * r.standard_normal((2, L))).astype(np.float32)
    one = REF.recording(refs, est, mix, 0, lags[0], D)
    two = REF.recording(refs, est, mix, 0, lags[0], D, lag_right=lags[1])
    got32 = REF.recording_sums(refs, est, mix, 0, lags[0], D, fp32=True)[0]
    assert REF.worst(got32, one["sums"], one["bound"][..., None]) <= 1.0
    miss = _misses(two["sums"], one["sums"], one["bound"][..., None])
    mg = _misses(two["gcc"], one["gcc"], one["E"][..., None])
    print("the right ear at its own lag: %d of %d sums missed, the largest by %.2g bounds; G by %.2g E; ITDs %s against %s us"
          % (int((miss > 1.0).sum()), miss.size, miss.max(), mg.max(), two["nine"][0, :3], one["nine"][0, :3]))
    assert miss.max() > 1.0 and mg.max() > 1.0
    assert one["nine"][0, :2].tolist() == [312.5, 500.0] and two["nine"][0, :2].tolist() == [312.5, 312.5]


@pytest.mark.parametrize("L,D,shift", REF.CASES)
@pytest.mark.parametrize("S", [2, 3])
def test_margins_of_the_gpu_cases(L, D, shift, S):
    """What lets the GPU test demand equal picks: every whole-recording peak has a margin above 2 E, and at most one window per case falls
    below it.  The planted delays are found, +-16 samples on the edge of the lags and 17 samples at the edge."""
    inputs, want = REF.case(L, D, shift, S)
    below = 0
    for r in range(REF.R):
        w = want[r]
        ratio = w["margin"] / (2.0 * w["E"])
        print("L = %d, D = %d, S = %d, recording %d: E %.2e .. %.2e, margin %.2e .. %.2e, margin / 2E %s" %
              (L, D, S, r, w["E"].min(), w["E"].max(), w["margin"].min(), w["margin"].max(), np.round(ratio, 2).tolist()))
        assert (ratio[0] > 1.0).all(), (r, ratio[0])
        below += int((ratio[1:] <= 1.0).any(axis=-1).sum())
        tgt, est = REF.PLANTED[r][0][0], REF.PLANTED[r][1]
        assert w["i"][0, 0] == 8 * tgt and w["i"][0, 1] == min(8 * est, 128) and w["i"][0, 2] == 8 * tgt      # (the mixture: its loudest source)
        assert w["nine"][0, 0] == 62.5 * tgt and w["nine"][0, 3] == abs(62.5 * min(est, 16) - 62.5 * tgt)
        assert w["gcc"].shape == (1 + w["sums"].shape[0], 3, 257) and not np.isnan(w["nine"]).any()
    assert below <= 1, below


def test_entry_point_refusals_name_score_itd_and_launch_nothing():
    """One refused call per shared check (csrc/score_stft.h, csrc/score_common.h).  Refusals return before any HIP call, so this runs
    without a GPU (the style of test_cabi.py's scorer refusals)."""
    lib = _lib.load()
    p, null = ctypes.c_void_p(256), None          # never dereferenced
    n0 = lib.m2h_launch_count()

    def call(refs=p, est=p, mix=p, target=None, target0=0, dft=p, out=p, R=2, S=3, L=100, lag=None, D=0):
        return lib.m2h_score_itd(refs, 600, 200, 100, est, 200, 100, mix, 200, 100, target, target0, dft, out, R, S, L, lag, D, None)

    rows = [(dict(refs=null), b"null pointer"), (dict(est=null), b"null pointer"), (dict(mix=null), b"null pointer"), (dict(out=null), b"null pointer"),
            (dict(dft=null), b"null pointer (dft)"), (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(R=0), b"R = 0"), (dict(L=0), b"L = 0"),
            (dict(lag=p, D=50, L=100), b"L = 100 samples; at least 2 D + 1 = 101"), (dict(D=4), b"a null pointer needs D = 0"),
            (dict(lag=p), b"a lag table needs D >= 1"), (dict(lag=p, D=8193), b"D = 8193"), (dict(target0=3), b"target = 3"),
            (dict(target0=-1), b"target = -1"), (dict(out=ctypes.c_void_p(260)), b"out must be 8-byte aligned"), (dict(L=2 ** 31 * 16000), b"2^31 - 1")]
    for kw, text in rows:
        assert call(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert msg.startswith(b"score_itd: ") and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_itd_gcc_refusals_launch_nothing():
    lib = _lib.load()
    p, null, odd = ctypes.c_void_p(256), None, ctypes.c_void_p(260)
    n0 = lib.m2h_launch_count()

    def call(sums=p, table=p, gcc=p, rows=3, k_lo=6, k_hi=256):
        return lib.m2h_itd_gcc(sums, table, gcc, rows, k_lo, k_hi, None)

    rows = [(dict(sums=null), b"null pointer"), (dict(table=null), b"null pointer"), (dict(gcc=null), b"null pointer"),
            (dict(k_lo=-1), b"k_lo = -1"), (dict(k_lo=6, k_hi=6), b"k_hi = 6"), (dict(k_lo=7, k_hi=6), b"k_lo = 7"), (dict(k_hi=257), b"k_hi = 257"),
            (dict(rows=0), b"rows = 0"), (dict(rows=2 ** 31), b"rows = 2147483648"),
            (dict(sums=odd), b"8-byte aligned"), (dict(table=odd), b"8-byte aligned"), (dict(gcc=odd), b"8-byte aligned")]
    for kw, text in rows:
        assert call(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert msg.startswith(b"itd_gcc: ") and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_scorer_refuses_mono_other_tiles_and_a_non_bool_before_any_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    scorer = SC.Scorer("cuda:0")                                                        # (no GPU call is made by the constructor or the checks)
    z = torch.zeros
    with pytest.raises(ValueError, match="itd=True .* needs C = 2 channels, got C = 1"):
        scorer.score(z(2, 50), z(2, 3, 50), z(2, 2, 50), itd=True)
    with pytest.raises(ValueError, match="itd=True .* needs C = 2 channels, got C = 1"):
        scorer.score(z(2, 1, 50), z(2, 3, 1, 50), z(2, 2, 50), itd=True)
    for tile in (7, 15999, 32000):
        with pytest.raises(ValueError, match="itd=True needs tile = 16000 .*got %d" % tile):
            scorer.score(z(2, 2, 50), z(2, 3, 2, 50), z(2, 2, 50), itd=True, tile=tile)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError, match="itd must be a bool, got %r" % (bad,)):
            scorer.score(z(2, 2, 50), z(2, 3, 2, 50), z(2, 2, 50), itd=bad)
    with pytest.raises(ValueError, match="estimate must live on cuda:0, got cpu"):
        scorer.score(z(2, 2, 50), z(2, 3, 2, 50), z(2, 2, 50), itd=True)
    assert scorer._itd is None and lib.m2h_launch_count() == n0
