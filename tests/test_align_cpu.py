"""CPU: the pure-Python and torch parts of the Scorer's alignment (m2h.audio.score.align_plan, lags_from_corr, every refusal), and a check
of the reference alone (tests/align_ref.py) for every case tests/test_gpu_align.py uses: the whole-recording margin -- largest |c| minus
second largest -- exceeds 2 E, twice the bound of the correlation it is taken from, so the GPU's lag must equal the reference's; of the
track's windows at most one per case (and recording, channel) may fall below 2 E, and those are not compared.
"""
import numpy as np
import pytest
import torch

import align_ref as AREF
from m2h.audio import score as SC


def _plan_literal(L, D, tile, window, hop):
    """align_plan restated: the region [D, L - D) cut into tiles, windows counted in tiles"""
    Lr = L - 2 * D
    J = -(-Lr // tile)
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    tiles = [(min(m * hop, J), min(m * hop + window, J)) for m in range(M)]
    return {"L": Lr, "tile": tile, "window": window, "hop": hop, "J": J, "M": M, "tiles": tiles, "offset": D,
            "samples": [(D + min(j0 * tile, Lr), D + min(j1 * tile, Lr)) for j0, j1 in tiles]}


@pytest.mark.parametrize("L,D,tile,window,hop", [(40001, 300, 16000, 1, 1), (40001, 300, 16000, 2, 1), (16000 - 1 + 64, 32, 16000, 1, 1),
                                                 (16000 + 64, 32, 16000, 1, 1), (16000 + 1 + 64, 32, 16000, 1, 1), (32769, 8192, 16384, 1, 1),
                                                 (8, 3, 7, 1, 1), (76, 3, 7, 2, 5), (64384, 8192, 16000, 5, 2)])
def test_align_plan_against_a_literal_restatement(L, D, tile, window, hop):
    got = SC.align_plan(L, D, tile, window, hop)
    assert got == _plan_literal(L, D, tile, window, hop)
    assert got["samples"] == [(a + D, b + D) for a, b in SC.score_plan(L - 2 * D, tile, window, hop)["samples"]]
    assert got["samples"][0][0] == D and max(b for _, b in got["samples"]) <= L - D


def test_align_plan_one_tile_minus_one_one_tile_one_tile_plus_one():
    D, tile = 32, 16000
    assert [SC.align_plan(tile + k + 2 * D, D, tile)["J"] for k in (-1, 0, 1)] == [1, 1, 2]
    assert SC.align_plan(tile - 1 + 2 * D, D, tile)["samples"] == [(32, 16031)]
    assert SC.align_plan(tile + 2 * D, D, tile)["samples"] == [(32, 16032)]
    assert SC.align_plan(tile + 1 + 2 * D, D, tile)["samples"] == [(32, 16032), (16032, 16033)]


def align_refusals():
    """(exception, message pattern, keyword arguments of align_plan / Scorer.score on L = 40001) for every refusal of `align`"""
    return [
        (ValueError, r"align must be in 1 \.\. 8192 samples, got 0", dict(align=0)),
        (ValueError, r"align must be in 1 \.\. 8192 samples, got -5", dict(align=-5)),
        (ValueError, r"align must be in 1 \.\. 8192 samples, got 8193", dict(align=8193)),
        (ValueError, r"align must be in 1 \.\. 8192 samples, got True", dict(align=True)),
        (TypeError, r"align must be an int or None, got 2\.5", dict(align=2.5)),
        (ValueError, r"tile \+ 2 align = 16385 \+ 2 \* 8192 = 32769 exceeds the transform's 32768 points", dict(align=8192, tile=16385)),
        (ValueError, r"tile \+ 2 align = 32000 \+ 2 \* 385 = 32770 exceeds", dict(align=385, tile=32000)),
        (ValueError, r"tile must be at least 1, got 0", dict(align=3, tile=0)),
    ]


def test_align_plan_refusals():
    for exc, pattern, kw in align_refusals():
        kw = dict(kw)
        with pytest.raises(exc, match=pattern):
            SC.align_plan(40001, kw.pop("align"), **kw)
    with pytest.raises(ValueError, match=r"L = 601 samples; align = 300 needs at least 2 \* 300 \+ 2 = 602"):
        SC.align_plan(601, 300)
    assert SC.align_plan(602, 300)["samples"] == [(300, 302)]
    assert SC.align_plan(32768, 8192, 16384)["J"] == 1                                  # both limits met exactly


def test_scorer_refuses_before_the_device_is_touched():
    sc = SC.Scorer(torch.device("cuda", 0))
    z = lambda *shape: torch.zeros(shape)   # noqa: E731
    ok = dict(estimate=z(2, 40001), references=z(2, 3, 40001), mixture=z(2, 2, 40001))
    for exc, pattern, kw in align_refusals():
        with pytest.raises(exc, match=pattern):
            sc.score(**dict(ok, **kw))
    with pytest.raises(ValueError, match=r"L = 50 samples; align = 25 needs at least 2 \* 25 \+ 2 = 52"):
        sc.score(estimate=z(2, 50), references=z(2, 3, 50), mixture=z(2, 2, 50), align=25)
    with pytest.raises(ValueError, match="estimate must live on cuda:0, got cpu"):       # everything else in order: the host tensor is named
        sc.score(**dict(ok, align=300))
    for bad in (0, -1, True):
        with pytest.raises(ValueError, match="max_corr_bytes must be positive"):
            SC.Scorer(torch.device("cuda", 0), max_corr_bytes=bad)


def test_kernel_argument_errors_need_no_gpu():
    """Every argument error of m2h_align_corr and m2h_score_gram_lag: a negative status, a message, nothing launched."""
    import ctypes
    from m2h import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)          # never dereferenced: the call fails before any launch
    n0 = lib.m2h_launch_count()

    def corr(refs=p, est=p, target=None, target0=0, tw=p, out=p, R=2, S=3, C=1, L=100, tile=10, D=5):
        return lib.m2h_align_corr(refs, 300, 100, 0, est, 100, 0, target, target0, tw, out, R, S, C, L, tile, D, None)

    for kw, text in ((dict(refs=None), b"null pointer"), (dict(est=None), b"null pointer"), (dict(tw=None), b"null pointer"), (dict(out=None), b"null pointer"),
                     (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(C=0), b"C = 0"), (dict(C=3), b"C = 3"), (dict(R=0), b"R = 0"), (dict(R=65536), b"R = 65536"),
                     (dict(D=0), b"D = 0"), (dict(D=8193), b"D = 8193"), (dict(tile=0), b"tile = 0"), (dict(L=1 << 40, tile=1), b"exceed a grid"), (dict(tile=32759), b"tile + 2 D = 32759 + 2 * 5"),
                     (dict(L=11), b"L = 11 samples; at least 2 D + 2 = 12"), (dict(target0=3), b"target = 3"), (dict(target0=-1), b"target = -1"),
                     (dict(tw=ctypes.c_void_p(260)), b"8-byte aligned"), (dict(out=ctypes.c_void_p(260)), b"8-byte aligned")):
        assert corr(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert b"align_corr" in msg and text in msg, (kw, msg)

    def gram(refs=p, est=p, mix=p, out=p, lag=p, R=2, S=3, C=1, L=100, tile=10, D=5):
        return lib.m2h_score_gram_lag(refs, 300, 100, 0, est, 100, 0, mix, 200, 100, out, R, S, C, L, tile, lag, D, None)

    for kw, text in ((dict(refs=None), b"null pointer"), (dict(est=None), b"null pointer"), (dict(mix=None), b"null pointer"), (dict(out=None), b"null pointer"),
                     (dict(lag=None), b"null pointer"), (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(C=0), b"C = 0"), (dict(C=3), b"C = 3"),
                     (dict(R=0), b"R = 0"), (dict(D=0), b"D = 0"), (dict(D=8193), b"D = 8193"), (dict(tile=0), b"tile = 0"),
                     (dict(L=10), b"L = 10 samples; at least 2 D + 1 = 11"), (dict(R=1 << 20, L=1 << 40, tile=1), b"exceed a grid")):
        assert gram(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert b"score_gram_lag" in msg and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_lags_from_corr():
    D = 4
    c = torch.zeros((7, 2 * D + 1), dtype=torch.float64)
    c[1, 0] = 2.0                                                                       # a peak at -D
    c[2, 2 * D] = 2.0                                                                   # a peak at +D
    c[3, D + 2] = -3.0                                                                  # a negative peak wins by its magnitude
    c[3, D - 1] = 2.0
    c[4, D - 3], c[4, D + 3] = 1.0, 1.0                                                 # equal maxima at -3 and +3: the negative one
    c[5, D - 3], c[5, D + 2] = -1.0, 1.0                                                # equal maxima at -3 and +2: the smaller |d|
    c[6, :] = 5.0                                                                       # all equal: 0
    c[6, D + 1] = -5.0
    got = SC.lags_from_corr(c)
    assert got.dtype == torch.int32 and got.tolist() == [0, -D, D, 2, -3, 2, 0]
    assert got.tolist() == AREF.lag_of(c.numpy()).tolist()
    assert SC.lags_from_corr(c.reshape(7, 1, 2 * D + 1).expand(7, 3, 2 * D + 1)).tolist() == [[v] * 3 for v in got.tolist()]
    assert SC.lags_from_corr(torch.zeros((1,), dtype=torch.float64)).tolist() == 0       # D = 0: one column
    r = np.random.default_rng(0)
    for D in (1, 3, 300):
        x = np.round(r.standard_normal((50, 2 * D + 1)) * 3)                            # small integers: many ties
        assert SC.lags_from_corr(torch.from_numpy(x)).tolist() == AREF.lag_of(x).tolist()
    with pytest.raises(TypeError, match="float64"):
        SC.lags_from_corr(c.float())
    with pytest.raises(ValueError, match="2 D \\+ 1 lags, not 8"):
        SC.lags_from_corr(c[:, :8])


def test_twiddle_helper_is_the_table_the_auralizer_had():
    """the shared builder restated: exp(-2 pi i k / 32768) in float64, rounded to fp32, then the stage-ordered copy"""
    from m2h.audio.twiddles import packed_twiddles
    t = packed_twiddles()
    M = 16384
    k = np.arange(M, dtype=np.float64)
    want = np.stack([np.cos(2.0 * np.pi * k / 32768), -np.sin(2.0 * np.pi * k / 32768)], axis=1).astype(np.float32)
    assert t.dtype == np.float32 and t.shape == (2, M, 2) and np.array_equal(t[0], want)
    for s in range(14):
        half = M >> (s + 1)
        assert np.array_equal(t[1, M - (M >> s):M - (M >> s) + half], want[(np.arange(half) << s) * 2])


def test_direct_sums_and_the_fft_route_of_the_reference_agree():
    case = AREF.CASES[0]
    refs, est, _, _ = AREF.case_inputs(case)
    a = AREF.corr_direct(refs[0, 0, 0], est[0, 0], case["D"], case["tile"], fft=False)
    b = AREF.corr_direct(refs[0, 0, 0], est[0, 0], case["D"], case["tile"], fft=True)
    scale = AREF.tile_bound(refs[0, 0, 0], est[0, 0], case["D"], case["tile"]) / AREF.PRODUCT_BOUND
    d = float((np.abs(a - b) / scale[:, None]).max())
    print("corr_direct, D = 300: longdouble sums against float64 scipy.fft: %.2e of |s| |x|" % d)
    assert d < 1e-14


@pytest.mark.parametrize("case", AREF.CASES, ids=AREF.case_id)
def test_reference_margins_of_the_gpu_cases(case):
    refs, est, _, _ = AREF.case_inputs(case)
    D, tile = case["D"], case["tile"]
    for r in range(AREF.R):
        for c in range(case["C"]):
            s, x = refs[r, 0, c], est[r, c]
            corr = AREF.window_sums(AREF.corr_direct(s, x, D, tile))
            E = AREF.window_sums(AREF.tile_bound(s, x, D, tile))
            margin, peak = AREF.margin_of(corr), np.abs(corr).max(axis=-1)
            lags = AREF.lag_of(corr)
            print("%s r=%d c=%d: lag %d (planted %d); relative margin: whole %.3g, smallest window %.3g; 2 E / peak %.2g" % (
                AREF.case_id(case), r, c, lags[0], case["lags"][r][c], margin[0] / peak[0], (margin[1:] / peak[1:]).min(), 2 * E[0] / peak[0]))
            assert lags[0] == case["lags"][r][c] or not case.get("recovered", True)     # the planted lag is the reference's whole-recording lag
            assert margin[0] > 2 * E[0]
            assert int((margin[1:] <= 2 * E[1:]).sum()) <= 1
