"""The Scorer's interaural cues without a GPU: the bound of tests/spatial_ref.py (it admits a correct fp32 implementation, the kernel's
folded arithmetic on spectral_table() included, and rejects the defects a fused binaural kernel can have), the definition's properties
and sign convention, the float64 algebra of spatial_from_sums, and the refusals of m2h_score_spatial and Scorer.score(spatial=True).

Measured (worst error / bound, misses of the planted defects): DESIGN.md §8.9."""
import ctypes

import numpy as np
import pytest
import torch

import score_ref
import spatial_ref as REF
import spectral_ref as SR
from m2h import _lib
from m2h.audio import score as SC

_cases = {}


def case(name):
    """the three binaural signals ((gL, gR), (eL, eR), (bL, bR)) as float64 rows; made once, shared and read-only"""
    if name not in _cases:
        if name == "clicks":
            refs, est, mix = REF.click_pairs()
        elif name == "binaural":
            refs, est, mix = REF.binaural()
        else:
            refs, est, mix = score_ref.inputs(2, name, 3, 2)
        _cases[name] = REF.signals(refs, est, mix)
        for pair in _cases[name]:
            for a in pair:
                a.setflags(write=False)
    return _cases[name]


_wants = {}


def want_of(name):
    if name not in _wants:
        _wants[name] = REF.tile_sums(case(name), 0)
        for a in _wants[name]:
            a.setflags(write=False)
    return _wants[name]


@pytest.mark.parametrize("name", [5, 700, 15999, 16000, "clicks", "binaural"])
def test_float32_restatement_stays_within_the_bound(name):
    want, bound = want_of(name)
    w = REF.worst(REF.tile_sums32(case(name), 0), want, bound)
    print("float32 restatement, %s: worst error / bound %.3e" % (name, w))
    assert want.shape == (3, 32, 4) and w <= 1.0
    big = want[:, :, :2] > 1e-3 * want[:, :, :2].max()                                   # the bound resolves the energies of every band that carries any
    assert (bound[:, :, :2][big] <= 1e-3 * want[:, :, :2][big]).all()


@pytest.mark.parametrize("name", [700, 16000, "clicks", "binaural"])
def test_the_kernels_folded_arithmetic_stays_within_the_bound(name):
    want, bound = want_of(name)
    got = REF.sums32([[SR.fold_on_the_table(SR.second(x, 0), SC.spectral_table()) for x in pair] for pair in case(name)])
    w = REF.worst(got, want, bound)
    print("folded table, %s: worst error / bound %.3e" % (name, w))
    assert w <= 1.0


def _sums(g, e, b):
    """float64 tile sums [3, 32, 4] of three [2, n] signals"""
    return REF.tile_sums(((g[0], g[1]), (e[0], e[1]), (b[0], b[1])), 0)[0]


def test_definition_properties():
    refs, est, mix = (np.asarray(a, np.float64) for a in REF.binaural(seed=2, L=8000))
    g, b = refs[0], mix
    w = REF.weights(_sums(g, g, b))
    ild_g = REF.cues(_sums(g, g, b))[0, :, 0]
    # E = G: the three errors are exactly 0, the improvements are the baseline's errors
    m = REF.metrics(_sums(g, g, b))
    assert (m[:3] == 0).all() and (m[6:] == m[3:6]).all() and (m[3:6] > 0).all()
    # one factor on both ears of E changes nothing
    m1, m3 = REF.metrics(_sums(g, est, b)), REF.metrics(_sums(g, 3.0 * est, b))
    assert np.abs(m3 - m1).max() <= 1e-12 and (m1[:3] > 0).all()
    # E's ears swapped: ILD_E = -ILD_G
    ms = REF.metrics(_sums(g, g[::-1], b))
    assert abs(ms[0] - (w * np.abs(2.0 * ild_g)).sum() / w.sum()) <= 1e-12
    # E = the target's mono downmix in both ears: no level difference, no phase difference, full coherence
    mono = 0.5 * (g[0] + g[1])
    s = _sums(g, np.stack([mono, mono]), b)
    c = REF.cues(s)[1]
    assert REF.valid(s, 1).all() and np.abs(c[:, 0]).max() <= 1e-12 and np.abs(c[:, 1]).max() <= 1e-12 and np.abs(c[:, 2] - 1.0).max() <= 1e-12
    assert abs(REF.metrics(s)[0] - (w * np.abs(ild_g)).sum() / w.sum()) <= 1e-12


def test_sign_convention_ipd_is_positive_when_the_right_ear_is_late():
    r = np.random.default_rng(4)
    x = r.standard_normal(SR.TILE + 4)
    g = np.stack([x[4:], x[:-4]])                                                       # right[t] = left[t - 4]
    ipd = REF.cues(_sums(g, g, g))[0, :, 1]
    lo, hi = 2.0 * np.pi * 16 * 4 / 1023, 2.0 * np.pi * 31 * 4 / 1023
    print("band 1: IPD %.4f rad in (%.4f, %.4f); band 0: %.4f" % (ipd[1], lo, hi, ipd[0]))
    assert lo < ipd[1] < hi and 0 < ipd[0] < lo


def _aligned_case():
    """D = 64, one tile: the estimate's ears are the target's, late by 37 and 40 samples, plus noise -> (refs, est, mix, D, lags)"""
    D, lags, L = 64, (37, 40), 2 * 64 + 16000
    r = np.random.default_rng(11)
    refs = (0.1 * r.standard_normal((1, 2, L))).astype(np.float32)
    est = np.zeros((2, L), np.float32)
    for c in range(2):
        est[c, lags[c]:] = refs[0, c, :L - lags[c]]
    est += (0.001 * r.standard_normal(est.shape)).astype(np.float32)
    mix = (refs[0] + 0.05 * r.standard_normal((2, L))).astype(np.float32)
    return refs, est, mix, D, lags


DEFECTS = {
    "ears swapped": dict(swap_ears=True),
    "the conjugate on the wrong factor": dict(wrong_conj=True),
    "band edges one bin late": dict(edge=1),
    "the cross term summed as |L| |R|": dict(abs_cross=True),
    "E's right ear paired with G's left": dict(cross_pair=True),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_the_bound_rejects_the_defect(defect):
    want, bound = want_of("binaural")
    assert REF.worst(REF.tile_sums32(case("binaural"), 0), want, bound) <= 1.0
    miss = np.abs(REF.tile_sums32(case("binaural"), 0, **DEFECTS[defect]) - want) / bound
    print("%s: %d of %d sums missed, the largest by %.2g bounds" % (defect, int((miss > 1.0).sum()), miss.size, miss.max()))
    assert miss.max() > 1.0


def test_the_bound_rejects_each_ear_read_at_its_own_lag():
    refs, est, mix, D, lags = _aligned_case()
    want, bound = REF.tile_sums(REF.signals(refs, est, mix, 0, lags[0], D), 0)
    assert REF.worst(REF.tile_sums32(REF.signals(refs, est, mix, 0, lags[0], D), 0), want, bound) <= 1.0
    miss = np.abs(REF.tile_sums32(REF.signals(refs, est, mix, 0, lags[0], D, lag_right=lags[1]), 0) - want) / bound
    print("each ear at its own lag: %d of %d sums missed, the largest by %.2g bounds" % (int((miss > 1.0).sum()), miss.size, miss.max()))
    assert miss.max() > 1.0
    # and what the rule is for: at one lag the estimate's extra interaural delay of 3 samples is measured, at two lags it is cancelled
    one = REF.metrics(want)[1]
    two = REF.metrics(REF.tile_sums(REF.signals(refs, est, mix, 0, lags[0], D, lag_right=lags[1]), 0)[0])[1]
    print("ipd_err at one lag %.4f rad, at each ear's own lag %.4f rad" % (one, two))
    assert one > 0.1 and two < 0.1 * one          # (what is left at two lags is the estimate's noise, 40 dB down)


def test_spatial_from_sums_against_the_reference_algebra():
    r = np.random.default_rng(1)
    sums = r.uniform(0.5, 2.0, (2, 5, 3, 32, 4))
    sums[..., 2:] = (sums[..., 2:] - 1.25) * np.sqrt(sums[..., 0:1] * sums[..., 1:2]) * 0.5       # |cross| <= sqrt(PL PR)
    sums = sums * 10.0 ** r.uniform(-6, 6, (2, 5, 1, 32, 1))
    sums[0, 1, 0, 3] = 0.0                                                               # a silent target band
    sums[0, 2, 1, 4, 1] = 0.0                                                            # the estimate's right ear silent in band 4
    sums[1, 0, 2, 31, 0] = 0.0                                                           # the mixture's left ear silent in band 31
    sums[1, 3, 0, :, :2] = 0.0                                                           # a silent target: no valid band
    got, cues = SC.spatial_from_sums(torch.from_numpy(sums))
    want = REF.metrics(sums)
    assert tuple(SC.SPATIAL_ORDER) == REF.ORDER and SC.SPATIAL_BANDS == REF.NB and SC.SPATIAL_IPD_BANDS == REF.IPD_BANDS
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 5, 9) and tuple(cues.shape) == (2, 5, 3, 32, 3)
    assert np.isnan(want[1, 3]).all() and bool(torch.isnan(got[1, 3]).all())
    keep = np.ones((2, 5), bool)
    keep[1, 3] = False
    assert np.isfinite(want[keep]).all() and np.abs(got.numpy()[keep] / want[keep] - 1.0).max() <= 1e-12
    ok = np.isfinite(REF.cues(sums))
    assert ok.mean() > 0.95 and np.abs(cues.numpy()[ok] - REF.cues(sums)[ok]).max() <= 1e-12
    # the skipped bands really are skipped: the same sums without them (weight 0) give the same numbers
    less = sums.copy()
    less[0, 2, :, 4] = 0.0
    assert np.abs(SC.spatial_from_sums(torch.from_numpy(less))[0].numpy()[0, 2, :3] / want[0, 2, :3] - 1.0).max() <= 1e-12
    # a difference across the branch cut is wrapped: IPD_G = 3, IPD_E = -3 are 2 pi - 6 apart
    s = np.ones((3, 32, 4))
    s[0, :, 2:], s[1, :, 2:] = (np.cos(3.0), np.sin(3.0)), (np.cos(-3.0), np.sin(-3.0))
    assert abs(float(SC.spatial_from_sums(torch.from_numpy(s))[0][1]) - (2.0 * np.pi - 6.0)) <= 1e-12
    with pytest.raises(TypeError, match="float64"):
        SC.spatial_from_sums(torch.zeros(3, 32, 4))
    with pytest.raises(ValueError, match=r"\[3, 32, 4\]"):
        SC.spatial_from_sums(torch.zeros(3, 16, 4, dtype=torch.float64))


def test_entry_point_refusals_name_score_spatial_and_launch_nothing():
    """Refusals return before any HIP call, so this runs without a GPU (the style of test_cabi.py's scorer refusals)."""
    lib = _lib.load()
    p, null = ctypes.c_void_p(256), None          # never dereferenced
    n0 = lib.m2h_launch_count()

    def call(refs=p, est=p, mix=p, target=None, target0=0, dft=p, out=p, R=2, S=3, L=100, lag=None, D=0):
        return lib.m2h_score_spatial(refs, 600, 200, 100, est, 200, 100, mix, 200, 100, target, target0, dft, out, R, S, L, lag, D, None)

    rows = [(dict(refs=null), b"null pointer"), (dict(est=null), b"null pointer"), (dict(mix=null), b"null pointer"), (dict(out=null), b"null pointer"),
            (dict(dft=null), b"null pointer (dft)"), (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(R=0), b"R = 0"), (dict(L=0), b"L = 0"),
            (dict(lag=p, D=50, L=100), b"L = 100"), (dict(D=4), b"D = 4"), (dict(lag=p), b"D = 0"), (dict(lag=p, D=8193), b"D = 8193"),
            (dict(target0=3), b"target = 3"), (dict(target0=-1), b"target = -1"), (dict(out=ctypes.c_void_p(260)), b"8-byte aligned"),
            (dict(L=2 ** 31 * 16000), b"2^31 - 1")]
    for kw, text in rows:
        assert call(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert msg.startswith(b"score_spatial: ") and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_scorer_refuses_mono_other_tiles_and_host_tensors_before_any_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    scorer = SC.Scorer("cuda:0")                                                        # (no GPU call is made by the constructor or the checks)
    z = torch.zeros
    with pytest.raises(ValueError, match="spatial=True .* needs C = 2 channels, got C = 1"):
        scorer.score(z(2, 50), z(2, 3, 50), z(2, 2, 50), spatial=True)
    with pytest.raises(ValueError, match="spatial=True .* needs C = 2 channels, got C = 1"):
        scorer.score(z(2, 1, 50), z(2, 3, 1, 50), z(2, 2, 50), spatial=True)
    for tile in (7, 15999, 32000):
        with pytest.raises(ValueError, match="spatial=True needs tile = 16000 .*got %d" % tile):
            scorer.score(z(2, 2, 50), z(2, 3, 2, 50), z(2, 2, 50), spatial=True, tile=tile)
    with pytest.raises(ValueError, match="estimate must live on cuda:0, got cpu"):
        scorer.score(z(2, 2, 50), z(2, 3, 2, 50), z(2, 2, 50), spatial=True)
    assert lib.m2h_launch_count() == n0
