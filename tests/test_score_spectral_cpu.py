"""The Scorer's STFT distance without a GPU: the float64 algebra of spectral_from_sums, the bound of tests/spectral_ref.py (it admits a
correct fp32 implementation and rejects the defects a fused kernel can have), the transform table of m2h_score_spectral with its fold,
and the one-second relation to the reference's STFT_L2_distance."""
import numpy as np
import pytest
import torch

import m2h_oracle as O
import score_ref
import spectral_ref as REF
from m2h.audio import score as SC

_cases = {}


def case(name):
    """(g, e, b) float64 rows of one channel; made once, shared and read-only"""
    if name not in _cases:
        if name == "clicks":
            refs, est, mix = REF.clicks()
        elif name == "clicks700":                                                       # a short tile: the clicks' last 700 samples
            refs, est, mix = (a[..., REF.TILE - 700:] for a in REF.clicks())
        else:
            L, snr43 = name
            refs, est, mix = score_ref.inputs(2, L, 3, 1, snr43)
        _cases[name] = REF.signals(refs, est, mix, 0)
        for a in _cases[name]:
            a.setflags(write=False)
    return _cases[name]


def test_spectral_from_sums_against_the_direct_definition():
    r = np.random.default_rng(1)
    sums = r.uniform(0.5, 2.0, (2, 2, 5, 7)) * 10.0 ** r.uniform(-6, 6, (2, 2, 5, 1))
    Q = np.array([3.0, 1.0, 2.0, 2.0, 1.0])
    got = SC.spectral_from_sums(torch.from_numpy(sums), torch.from_numpy(Q))
    want = REF.metrics(sums, Q)
    assert tuple(SC.SPECTRAL_ORDER) == REF.ORDER and got.dtype == torch.float64 and tuple(got.shape) == (2, 2, 5, 8)
    assert np.abs(got.numpy() / want - 1.0).max() <= 1e-12
    # a number for Q; an empty window (Q = 0, all sums 0) is NaN; a silent target leaves the distances finite and sc NaN or inf
    assert torch.equal(SC.spectral_from_sums(torch.from_numpy(sums[..., :1, :]), 3), got[..., :1, :])
    assert bool(torch.isnan(SC.spectral_from_sums(torch.zeros(7, dtype=torch.float64), 0)).all())
    silent = SC.spectral_from_sums(torch.tensor([0.0, 2.0, 3.0, 2.0, 2.0, 3.0, 3.0], dtype=torch.float64), 1)
    assert bool(torch.isinf(silent[2])) and bool(torch.isfinite(silent[[0, 1, 3, 4, 6, 7]]).all())
    with pytest.raises(TypeError, match="float64"):
        SC.spectral_from_sums(torch.zeros(7), 1)
    with pytest.raises(ValueError, match="7 numbers"):
        SC.spectral_from_sums(torch.zeros(6, dtype=torch.float64), 1)


@pytest.mark.parametrize("name", [(5, False), (700, False), (15999, False), (16000, False), (16000, True), "clicks", "clicks700"])
def test_float32_restatement_stays_within_the_bound(name):
    g, e, b = case(name)
    want, bound = REF.tile_sums(g, e, b, 0)
    got = REF.tile_sums32(g, e, b, 0)
    w = REF.worst(got, want, bound)
    print("float32 restatement, %s: worst error / bound %.3e; bound / sum of stft_l2's %.3e" % (name, w, bound[3] / want[3]))
    assert w <= 1.0
    assert bound[3] <= 1e-2 * want[3]                                                   # the bound resolves the metric: far below stft_l2 itself


DEFECTS = {
    "constant instead of reflect padding": ("clicks", {"pad_mode": "constant"}),
    "frames one sample early": ("clicks", {"offset": -1}),
    "frames one sample late": ("clicks", {"offset": 1}),
    "no window": ("clicks", {"window": np.ones(REF.NFFT, np.float32)}),
    "symmetric instead of periodic Hann": ("clicks", {"window": REF.hann32(symmetric=True)}),
    "a short last tile reflected at L instead of zero-extended": ("clicks700", {"reflect_at": 700}),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_the_bound_rejects_the_defect(defect):
    name, kw = DEFECTS[defect]
    g, e, b = case(name)
    want, bound = REF.tile_sums(g, e, b, 0)
    miss = np.abs(REF.tile_sums32(g, e, b, 0, **kw) - want) / bound
    print("%s: smallest / largest miss over the seven sums %.2g / %.2g bounds" % (defect, miss.min(), miss.max()))
    assert miss.max() >= 10.0


@pytest.mark.parametrize("name", [(16000, False), "clicks", "clicks700"])
def test_the_folded_table_computes_the_definition(name):
    g, e, b = case(name)
    want, bound = REF.tile_sums(g, e, b, 0)
    got = REF.seven32(*[REF.fold_on_the_table(REF.second(x, 0), SC.spectral_table()) for x in (g, e, b)])
    w = REF.worst(got, want, bound)
    print("folded table, %s: worst error / bound %.3e" % (name, w))
    assert w <= 1.0


def test_one_second_relation_to_the_reference_distance():
    """stft_l2 of a one-second recording is the mono number of STFT_L2_distance fed from oracle.np_stft spectra"""
    refs, est, mix = score_ref.inputs(1, REF.TILE, 7)
    sums, bound = REF.recording_sums(refs, est, mix)
    G, E = O.np_stft(refs[0, 0]), O.np_stft(est[0])                                      # complex64 [F, T]
    assert G.shape == (REF.F, REF.T)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))[None, :, :, None]   # noqa: E731
    gt = torch.cat([t(np.abs(G)), t(np.angle(G))], dim=-1)
    zeros = torch.zeros((1, REF.F, REF.T, 2), dtype=torch.float64)
    dm = O.stft_l2_distance(zeros, zeros, torch.cat([gt, gt], dim=-1), t(np.abs(E)), gt)[1]
    want = REF.metrics(sums[0, 0], 1.0)[0]
    tol = REF.metrics_bound(sums[0, 0], bound[0, 0], 1.0)[0]
    print("STFT_L2_distance %.9e, stft_l2 %.9e, bound %.3e" % (float(dm), want, tol))
    assert abs(float(dm) - want) <= tol
