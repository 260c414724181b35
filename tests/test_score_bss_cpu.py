"""The Scorer's BSS-eval numbers without a GPU: the two numpy routes of tests/bss_ref.py against each other (which fixes TOL_BSS), the
properties the definition promises, the refusals of Scorer.score(..., bss=T), the plan, the torch solve on the CPU, and a mutant table."""
import numpy as np
import pytest
import torch

import bss_ref as B
import score_ref
from m2h import _lib
from m2h.audio import score as SC

SEED = 31
_cache = {}


def inputs(case, which="plain"):
    """(refs [S, C, L], est [C, L], mix [2, L]) of a case: score_ref.inputs, or with bss_ref's filtered estimate"""
    key = (case, which)
    if key not in _cache:
        L, tile, T, S, C = case
        refs, est, mix = score_ref.inputs(S, L, SEED, C)
        if which == "filtered":
            est = B.filtered_estimate(refs, mix, 7)
        _cache[key] = (refs, est, mix)
    return _cache[key]


def direct(case, which, route, window=1, hop=1, **kw):
    key = (case, which, route, window, hop, tuple(sorted(kw.items())))
    if key not in _cache:
        L, tile, T, S, C = case
        refs, est, mix = inputs(case, which)
        _cache[key] = B.bss_direct(refs, est, mix, 0, tile, window, hop, T, route=route, **kw)
    return _cache[key]


def estimates(case):
    return ("plain", "filtered") if case[0] >= 300 else ("plain",)      # the filtered estimate needs room for its 237 taps


def test_the_two_routes_agree_and_fix_the_tolerance():
    worst = 0.0
    for case in B.CASES:
        for which in estimates(case):
            for window, hop in ((1, 1), (2, 1)):
                a, b = direct(case, which, "a", window, hop), direct(case, which, "b", window, hop)
                assert not np.isnan(a[0][:, (0, 2, 3, 5, 6, 8)]).any(), (case, which)      # (S = 1: sir is +inf and siri inf - inf)
                d = max(B.max_err(a[0], b[0]), B.max_err(a[1], b[1]))
                print("routes a / b  %-28s %-8s window %d: %.2e dB" % (case, which, window, d))
                worst = max(worst, d)
    print("worst spread %.3e dB, SPREAD_BSS %.1e, TOL_BSS %.2e" % (worst, B.SPREAD_BSS, B.TOL_BSS))
    assert worst <= B.SPREAD_BSS <= 8 * worst               # the constant is held to the measurement (1.33e-12), from both sides
    assert B.TOL_BSS == 64 * B.SPREAD_BSS and B.TOL_BSS <= score_ref.TOL_GPU
    assert SC.BSS_ORDER == B.BSS_ORDER


@pytest.mark.parametrize("case", B.CASES)
def test_the_components_are_orthogonal(case):
    """|s_t|^2 + |P - s_t|^2 + |x - P|^2 = |x|^2 over the whole recording, tail included (measured: 2e-15 relative)"""
    L, tile, T, S, C = case
    refs, est, mix = inputs(case)
    for c in range(C):
        sums = B.channel_sums(refs, est, mix, c, 0, tile, 1, 1, T)[0]
        s, x, b = B.signals(refs, est, mix, c)
        for q, y in ((0, x), (5, b)):
            total = sums[q] + sums[q + 2] + sums[q + 4]
            assert abs(total - (y ** 2).sum()) <= 1e-13 * (y ** 2).sum(), (case, c, q, total / (y ** 2).sum() - 1)


def test_a_filtered_target_is_a_perfect_estimate():
    """x = s_j through any FIR of at most T taps: SDR and SAR above 150 dB (float64 estimate; the target ends in T - 1 zeros so that the
    filter's tail lies inside the recording)"""
    L, T, S = 3000, 64, 3
    refs, _, mix = score_ref.inputs(S, L, SEED, 1)
    refs = refs.copy()
    refs[1, 0, L - T + 1:] = 0.0
    r = np.random.default_rng(5)
    for taps in (1, 17, T):
        est = np.convolve(refs[1, 0].astype(np.float64), r.standard_normal(taps))[None, :L]
        for route in ("a", "b"):
            whole, _ = B.bss_direct(refs, est, mix, 1, 1000, 1, 1, T, route=route)
            print("filtered target, %d taps, route %s: sdr %.1f dB, sar %.1f dB" % (taps, route, whole[0, 0], whole[0, 2]))
            assert whole[0, 0] > 150 and whole[0, 2] > 150


def test_sdr_does_not_depend_on_the_estimates_gain():
    case = (4001, 16000, 512, 3, 1)
    refs, est, mix = score_ref.inputs(3, 4001, SEED, 1)
    a = B.bss_direct(refs, est.astype(np.float64), mix, 0, 1000, 1, 1, 128)
    b = B.bss_direct(refs, 0.37 * est.astype(np.float64), mix, 0, 1000, 1, 1, 128)
    assert B.max_err(a[0][:, :3], b[0][:, :3]) <= B.TOL_BSS and B.max_err(a[1][..., :3], b[1][..., :3]) <= B.TOL_BSS, case


def test_the_filtered_estimate_is_the_defect_si_sdr_has():
    for case in B.CASES:
        if "filtered" not in estimates(case):
            continue
        L, tile, T, S, C = case
        refs, est, mix = inputs(case, "filtered")
        whole = direct(case, "filtered", "a")[0]
        for c in range(C):
            si_sdr = score_ref.score_window_direct(refs, est, mix, c, 0, 0, L)[0]
            print("filtered estimate %-28s channel %d: si_sdr %.2f dB, bss sdr %.2f dB" % (case, c, si_sdr, whole[c, 0]))
            assert whole[c, 0] - si_sdr > 10


def test_the_gram_from_lags_is_the_gram_of_the_shifted_references():
    refs, est, mix = score_ref.inputs(3, 2000, SEED, 1)
    s, _, _ = B.signals(refs, est, mix, 0)
    for route in ("a", "b"):
        G, E = B.gram_from_lags(B.lags(s, 64, route), 64), B.explicit_gram(s, 64)
        err = np.abs(G - E).max() / np.abs(E).max()
        print("gram from lags against the explicit gram, route %s: %.2e relative" % (route, err))
        assert err <= 1e-12                                  # measured 2.0e-15


def test_one_sided_lags_give_the_same_numbers_through_the_torch_solve():
    """SC.bss_filters on CPU tensors, fed the one-sided correlations of m2h_bss_corr's layout computed by numpy, against route a"""
    for case, which in (((40, 7, 8, 3, 2), "plain"), ((2000, 16000, 512, 3, 1), "filtered")):
        L, tile, T, S, C = case
        refs, est, mix = inputs(case, which)
        corr = np.zeros((1, C, S, S + 2, T))
        for c in range(C):
            s, x, b = B.signals(refs, est, mix, c)
            for i in range(S):
                for k, v in enumerate(list(s) + [x, b]):
                    corr[0, c, i, k] = B.xcorr(s[i], v, T)[T - 1:]
        h, ok = SC.bss_filters(torch.from_numpy(corr), 0)
        assert bool(ok.all())
        rows = []
        for c in range(C):
            s, x, b = B.signals(refs, est, mix, c)
            sums, _ = B.project_tiles(s, x, b, h[0, c].numpy(), 0, tile)
            rows.append(SC.bss_from_sums(torch.from_numpy(sums.sum(axis=0))).numpy())
        err = B.max_err(np.stack(rows), direct(case, which, "a")[0])
        print("torch solve on one-sided lags %-28s: %.2e dB" % (case, err))
        assert err <= B.TOL_BSS


def test_silent_references():
    """a silent interferer is left out (the numbers of the call without it); a silent target gives nine NaN"""
    refs, est, mix = score_ref.inputs(3, 1200, SEED, 1)
    quiet = refs.copy()
    quiet[2] = 0.0
    a = B.bss_direct(quiet, est, mix, 0, 500, 1, 1, 32)
    b = B.bss_direct(quiet[:2], est, mix, 0, 500, 1, 1, 32)
    assert B.max_err(a[0], b[0]) <= B.TOL_BSS and B.max_err(a[1], b[1]) <= B.TOL_BSS
    c = B.bss_direct(quiet, est, mix, 2, 500, 1, 1, 32)
    assert np.isnan(c[0]).all() and np.isnan(c[1]).all()
    corr = torch.zeros((1, 1, 2, 4, 8), dtype=torch.float64)
    corr[0, 0, 0, 0, 0] = 1.0
    h, ok = SC.bss_filters(corr, 1)                          # the target is silent: not ok, and nothing raises
    assert not bool(ok.any())
    assert bool(torch.isnan(SC.bss_from_sums(torch.ones((1, 1, 10), dtype=torch.float64), ok)).all())


def test_plan_and_tail_ownership():
    for Lr, tile, T in ((40, 7, 8), (16001, 16000, 512), (14, 7, 3)):
        for window, hop in ((1, 1), (2, 1), (1, 3)):
            J, wins = B.plan(Lr, tile, window, hop)
            p = SC.score_plan(Lr, tile, window, hop)
            assert (J, wins) == (p["J"], p["tiles"])
            seen = []
            for j in range(J):
                n0, n1 = B.owned(j, j + 1, J, Lr, tile, T)
                assert n0 == j * tile and n1 == (Lr + T - 1 if j == J - 1 else (j + 1) * tile)
                seen += list(range(n0, n1))
            assert seen == list(range(Lr + T - 1))           # every output sample has exactly one owner, the tail the last tile
            for j0, j1 in wins:
                n0, n1 = B.owned(j0, j1, J, Lr, tile, T)
                assert (n1 - n0 == 0) if j0 >= j1 else (n0 == j0 * tile and (n1 == Lr + T - 1) == (j1 == J))


def test_bad_bss_values_and_short_recordings_are_refused_before_any_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    scorer = SC.Scorer("cuda:0")                              # (constructing a Scorer touches no device)
    z = lambda *shape: torch.zeros(shape)                     # noqa: E731
    ok = dict(estimate=z(2, 2000), references=z(2, 3, 2000), mixture=z(2, 2, 2000))
    for bad in (True, False, 8.0, "8", (8,)):
        with pytest.raises(TypeError, match="bss must be an int .*got %s" % repr(bad).replace("(", r"\(").replace(")", r"\)")):
            scorer.score(bss=bad, **ok)
    for bad in (0, -1, 513, 10 ** 6):
        with pytest.raises(ValueError, match="bss must be in 1 .. 512 taps, got %d" % bad):
            scorer.score(bss=bad, **ok)
    with pytest.raises(ValueError, match=r"bss = 512 taps and S = 3 references need at least S \* bss = 1536 scored samples, got 600"):
        scorer.score(bss=512, estimate=z(2, 600), references=z(2, 3, 600), mixture=z(2, 2, 600))
    with pytest.raises(ValueError, match=r"need at least S \* bss = 1536 scored samples, got 1528"):
        scorer.score(bss=512, align=236, **ok)                # the region counts, not the recording
    with pytest.raises(ValueError, match="estimate must live on cuda:0, got cpu; the scorer has no CPU path"):
        scorer.score(bss=512, **ok)
    assert lib.m2h_launch_count() == n0


# Each defect planted in route a must miss the float64 definition by more than TOL_BSS on its case: (case, estimate, align D or 0, the miss in dB
# measured here).  `nolag` only exists under alignment: D = 8 with the estimate 3 and -2 samples late.
ALIGNED = ((56, 7, 8, 3, 2), 8, (3, -2))
MUTANT_TABLE = {
    "tail": ((40, 7, 8, 3, 2), "plain", 7.005),
    "lag_sign": ((40, 7, 8, 3, 2), "plain", 25.25),
    "st_joint": ((40, 7, 8, 3, 2), "plain", 12.65),
    "taps": ((40, 7, 8, 3, 2), "plain", 3.225),
    "means": ((40, 7, 8, 3, 2), "plain", 7.308),
    "border": ((16001, 16000, 512, 3, 2), "plain", 0.1362),
    "fp32corr": ((2000, 16000, 512, 3, 1), "filtered", 2.135e-5),
    "base_filters": ((40, 7, 8, 3, 2), "plain", 29.51),
    "nolag": (ALIGNED[0], "plain", 6.939),
}


def test_the_mutant_table_names_every_defect():
    assert tuple(MUTANT_TABLE) == B.MUTANTS


@pytest.mark.parametrize("mutant", B.MUTANTS)
def test_every_planted_defect_misses_the_definition(mutant):
    case, which, recorded = MUTANT_TABLE[mutant]
    L, tile, T, S, C = case
    refs, est, mix = inputs(case, which)
    kw = dict(D=ALIGNED[1], lags_=ALIGNED[2]) if case == ALIGNED[0] else {}
    good = B.bss_direct(refs, est, mix, 0, tile, 1, 1, T, **kw)
    bad = B.bss_direct(refs, est, mix, 0, tile, 1, 1, T, mutant=mutant, **kw)
    miss = max(B.max_err(bad[0], good[0]), B.max_err(bad[1], good[1]))
    print("mutant %-12s on %-28s misses by %.3e dB (recorded %.3e)" % (mutant, case, miss, recorded))
    assert miss > B.TOL_BSS
    assert 0.5 * recorded <= miss <= 2.0 * recorded                 # the table records what was measured
