"""GPU: the Scorer's alignment (m2h.audio.score, csrc/align.hip, m2h_score_gram_lag) against its float64 restatement (tests/align_ref.py).

Bounds.  The tile correlations against align_ref.corr_direct, every entry: |got - want| <= E(tile) = PRODUCT_BOUND |s_seg|_2 |x_seg|_2, the
project's bound for one product of the 32768-point fp32 transform (tests/render_ref.py) on the correlation's Cauchy-Schwarz scale.  The
lags: equal to the reference's wherever the reference's margin exceeds 2 E (tests/test_align_cpu.py shows that it does for every whole
recording used here).  The scores against score_aligned_f64: score_ref.TOL_GPU, as for the unaligned scorer.  The batch, the grouping, the
strides and the alignment of a row do not change the arithmetic or its order: those comparisons are bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref as AREF
import score_ref as REF
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = AREF.R
SCORED = [c for c in AREF.CASES if c["L"] - 2 * c["D"] > 2]       # (two samples have no score: every centred signal is a multiple of (1, -1))
SMALL = AREF.CASES[0]                                            # L = 40001, tile 16000, D = 300, two ears with their own lags


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scorer(dev):
    from m2h.audio.score import Scorer
    return Scorer(dev)


def _gpu(dev, *arrays):
    return [torch.tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]      # (a copy: the shared inputs are read-only)


def _args(ge, gr, gm, C):
    """the public shapes: [R, L] and [R, S, L] for C = 1"""
    return (ge[:, 0], gr[:, :, 0], gm) if C == 1 else (ge, gr, gm)


def _same(a, b):
    """bit for bit, NaN in the same places"""
    if a.dtype != torch.float64:
        return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))
    return a.shape == b.shape and bool(torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))) and \
        bool(torch.equal(torch.isnan(a), torch.isnan(b)))


def _same_result(a, b, keys=("whole", "track", "active", "lag", "lag_track")):
    return all(_same(a[k], b[k]) for k in keys)


_reference = {}


def reference(case):
    """per (r, c): the tile correlations [J, 2 D + 1] and their bounds [J] of the float64 restatement; computed once per case"""
    key = AREF.case_id(case)
    if key not in _reference:
        refs, est, _, _ = AREF.case_inputs(case)
        _reference[key] = {(r, c): (AREF.corr_direct(refs[r, 0, c], est[r, c], case["D"], case["tile"]),
                                    AREF.tile_bound(refs[r, 0, c], est[r, c], case["D"], case["tile"]))
                           for r in range(R) for c in range(case["C"])}
    return _reference[key]


@pytest.mark.parametrize("case", AREF.CASES, ids=AREF.case_id)
def test_tile_correlations_against_direct_sums(dev, scorer, case):
    refs, est, _, _ = AREF.case_inputs(case)
    gr, ge = _gpu(dev, refs, est)
    D, tile, C = case["D"], case["tile"], case["C"]
    got = ops.align_corr(gr, ge, 0, tile, D, scorer._twiddle_table())
    assert ops.last_kernel() == "align_corr"
    J = -(-(case["L"] - 2 * D) // tile)
    assert got.dtype == torch.float64 and tuple(got.shape) == (R, C, J, 2 * D + 1)
    assert torch.equal(got, ops.align_corr(gr, ge, 0, tile, D, scorer._twiddle_table()))                 # the same bits on every run
    got = got.cpu().numpy()
    worst = 0.0
    for (r, c), (want, E) in reference(case).items():
        err = np.abs(got[r, c] - want).max(axis=-1)
        worst = max(worst, float((err / E).max()))
        assert np.isfinite(got[r, c]).all() and (err <= E).all(), (r, c, (err / E).tolist())
    print("tile correlations %s: largest error %.3f of E = PRODUCT_BOUND |s| |x|  (%.2e of |s| |x|)" % (AREF.case_id(case), worst, worst * AREF.PRODUCT_BOUND))


@pytest.mark.parametrize("case", AREF.CASES, ids=AREF.case_id)
def test_lags_equal_the_references(dev, scorer, case):
    refs, est, mix, _ = AREF.case_inputs(case)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    D, tile, C = case["D"], case["tile"], case["C"]
    for window, hop in ((1, 1), (2, 1)):
        res = scorer.score(*_args(ge, gr, gm, C), tile=tile, window=window, hop=hop, align=D)
        M = res["plan"]["M"]
        assert res["lag"].dtype == torch.int32 and tuple(res["lag"].shape) == (R, C) and res["lag"].is_cuda
        assert res["lag_track"].dtype == torch.int32 and tuple(res["lag_track"].shape) == (R, C, M) and res["lag_track"].is_cuda
        assert res["plan"]["offset"] == D and res["plan"]["samples"][0][0] == D and tuple(res["track"].shape) == (R, C, M, 11)
        lag, track = res["lag"].cpu().numpy(), res["lag_track"].cpu().numpy()
        compared = 0
        for (r, c), (ct, E) in reference(case).items():
            corr, bound = AREF.window_sums(ct, window, hop), AREF.window_sums(E, window, hop)
            want = AREF.lag_of(corr)
            sure = AREF.margin_of(corr) > 2 * bound
            assert sure[0] and lag[r, c] == want[0], (r, c, lag[r, c], want[0])
            if case.get("recovered", True):
                assert lag[r, c] == case["lags"][r][c]                              # the planted lag, +-D included
            assert (track[r, c][sure[1:]] == want[1:][sure[1:]]).all(), (r, c, track[r, c].tolist(), want[1:].tolist())
            compared += int(sure[1:].sum())
        assert compared >= R * C * M - R * C                                            # at most one window per (r, c) left out


@pytest.mark.parametrize("case", SCORED, ids=AREF.case_id)
def test_scores_match_the_definition_and_the_unaligned_scorer_misses(dev, scorer, case):
    refs, est, mix, clean = AREF.case_inputs(case)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    D, tile, C = case["D"], case["tile"], case["C"]
    worst = 0.0
    for window, hop in ((1, 1), (2, 1)):
        res = scorer.score(*_args(ge, gr, gm, C), tile=tile, window=window, hop=hop, align=D)
        whole, track, lag = res["whole"].cpu().numpy(), res["track"].cpu().numpy(), res["lag"].cpu().numpy()
        for r in range(R):
            want_whole, want_track = AREF.score_aligned_f64(refs[r], est[r], mix[r], D, lag[r], 0, tile, window, hop)
            assert np.isfinite(want_whole).all()
            e = max(REF.max_err(whole[r], want_whole), REF.max_err(track[r], want_track))
            worst = max(worst, e)
            assert e <= REF.TOL_GPU, (window, hop, r, e)
    print("aligned scores %s: largest error %.3e dB of %.0e" % (AREF.case_id(case), worst, REF.TOL_GPU))
    # the defect the feature removes: the same shifted estimate scored without alignment misses the score of the estimate before the shift
    plain = scorer.score(*_args(ge, gr, gm, C), tile=tile)["whole"].cpu().numpy()
    for r in range(R):
        unshifted = REF.score_direct_f64(refs[r], clean[r], mix[r], 0, tile)[0]
        for c in range(C):
            if case["lags"][r][c] != 0:
                miss = float(np.abs(plain[r, c] - unshifted[c])[list(REF.WELL)].min())
                assert miss > REF.TOL_DEFECT, (r, c, miss)


def test_aligned_score_equals_the_score_of_hand_cut_slices(dev, scorer):
    for case in (SMALL, AREF.CASES[3], AREF.CASES[5]):
        refs, est, mix, _ = AREF.case_inputs(case)
        gr, ge, gm = _gpu(dev, refs, est, mix)
        D, tile, C, L = case["D"], case["tile"], case["C"], case["L"]
        res = scorer.score(*_args(ge, gr, gm, C), tile=tile, window=2, hop=1, align=D)
        lag = res["lag"].cpu().tolist()
        cut = torch.stack([torch.stack([ge[r, c, D + lag[r][c]:L - D + lag[r][c]] for c in range(C)]) for r in range(R)])
        by_hand = scorer.score(*_args(cut, gr[..., D:L - D], gm[..., D:L - D], C), tile=tile, window=2, hop=1)
        assert _same_result(res, by_hand, ("whole", "track", "active")), AREF.case_id(case)
        assert [(a - D, b - D) for a, b in res["plan"]["samples"]] == by_hand["plan"]["samples"]


def test_batching_and_grouping_change_no_bit(dev, scorer):
    from m2h.audio.score import Scorer
    refs, est, mix, _ = AREF.case_inputs(SMALL)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    D, tile = SMALL["D"], SMALL["tile"]
    res = scorer.score(ge, gr, gm, tile=tile, window=2, hop=1, align=D)
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), tile=tile, window=2, hop=1, align=D)
        assert all(_same(solo[k][0], res[k][r]) for k in ("whole", "track", "active", "lag", "lag_track")), r
    one_by_one = Scorer(dev, max_corr_bytes=1)                                         # every recording is above it: each goes alone
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    grouped = one_by_one.score(ge, gr, gm, tile=tile, window=2, hop=1, align=D)
    assert lib.m2h_launch_count() - n0 == 3 * R + 3                                     # R x (correlation, two window sums), the Gram, two window sums
    assert _same_result(grouped, res)
    # per-recording targets go to the kernel as device data: recording 1 estimates source 1
    est2 = np.stack([est[0], AREF.shifted((0.7 * refs[1, 1] + 0.1 * est[1]).astype(np.float32), -77)])
    ge2, = _gpu(dev, est2)
    both = scorer.score(ge2, gr, gm, target=[0, 1], tile=tile, align=D)
    assert both["lag"].cpu().tolist() == [SMALL["lags"][0], [-77, -77]]
    for r, t in enumerate((0, 1)):
        solo = scorer.score(ge2[r:r + 1], gr[r:r + 1], gm[r:r + 1], target=t, tile=tile, align=D)
        assert all(_same(solo[k][0], both[k][r]) for k in ("whole", "track", "active", "lag", "lag_track")), r
        want_whole, want_track = AREF.score_aligned_f64(refs[r], est2[r], mix[r], D, both["lag"][r].cpu().numpy(), t, tile)
        assert max(REF.max_err(both["whole"][r].cpu().numpy(), want_whole), REF.max_err(both["track"][r].cpu().numpy(), want_track)) <= REF.TOL_GPU


def test_strides_and_row_alignment_change_no_bit(dev, scorer):
    refs, est, mix, _ = AREF.case_inputs(SMALL)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    D, tile, C, L, S = SMALL["D"], SMALL["tile"], SMALL["C"], SMALL["L"], AREF.S
    res = scorer.score(ge, gr, gm, tile=tile, window=2, hop=1, align=D)
    # strided views against contiguous copies: references sliced out of a larger `images`, an estimate viewed from a larger buffer
    images = torch.zeros((R + 1, S + 2, C, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    assert _same_result(scorer.score(*views, tile=tile, window=2, hop=1, align=D), res)
    # odd L misaligns every second row of the contiguous tensors; the same data in buffers whose rows are all 16-byte aligned
    assert L % 4 == 1 and all(t.data_ptr() % 16 == 0 for t in (gr, ge, gm))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (3,), device=dev)], dim=-1)[..., :L]   # noqa: E731  (row stride L + 3 = 40004)
    assert _same_result(scorer.score(pad(ge), pad(gr), pad(gm), tile=tile, window=2, hop=1, align=D), res)
    # the mono form of the same call: channel 0 of the two-channel call
    mono = scorer.score(ge[:, 0], gr[:, :, 0], gm, tile=tile, window=2, hop=1, align=D)
    assert _same(mono["lag"], res["lag"][:, :1]) and _same(mono["lag_track"], res["lag_track"][:, :1])


def test_rows_past_two_to_the_31_elements(dev, scorer):
    """An estimate whose second row starts 2^31 + 8 elements after the first (a view of a larger buffer): the strides are 64-bit."""
    case = AREF.CASES[4]
    refs, est, mix, _ = AREF.case_inputs(case)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    L, stride = case["L"], 2 ** 31 + 8
    buf = torch.empty((stride + L + 8,), device=dev)
    view = buf.as_strided((R, 1, L), (stride, L, 1), 3)
    view.copy_(ge)
    assert view.stride(0) > 2 ** 31 and view.data_ptr() % 16 != 0
    far = scorer.score(view, gr, gm, tile=case["tile"], align=case["D"])
    near = scorer.score(ge, gr, gm, tile=case["tile"], align=case["D"])
    assert _same_result(far, near) and near["lag"].cpu().tolist() == case["lags"]


def test_the_old_entry_point_is_unchanged_and_is_the_new_one_at_zero_lag(dev):
    refs, est, mix, _ = AREF.case_inputs(SMALL)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    D, tile, L = SMALL["D"], SMALL["tile"], SMALL["L"]
    before = ops.score_gram(gr, ge, gm, tile)
    assert ops.last_kernel() == "score_gram"
    zero = torch.zeros((R, SMALL["C"]), dtype=torch.int32, device=dev)
    lagged = ops.score_gram_lag(gr, ge, gm, tile, zero, D)
    assert ops.last_kernel() == "score_gram_lag"
    after = ops.score_gram(gr, ge, gm, tile)
    assert torch.equal(before, after)
    assert torch.equal(lagged, ops.score_gram(gr[..., D:L - D], ge[..., D:L - D], gm[..., D:L - D], tile))
    # a lag outside [-D, D] (device data: a NaN-born value, say) is clamped, never followed out of the row
    wild = torch.tensor([[2 ** 31 - 1, -2 ** 31], [D + 1, -D - 1]], dtype=torch.int32).to(dev)
    edge = torch.tensor([[D, -D], [D, -D]], dtype=torch.int32).to(dev)
    assert torch.equal(ops.score_gram_lag(gr, ge, gm, tile, wild, D), ops.score_gram_lag(gr, ge, gm, tile, edge, D))
    # and against the float64 Gram of the slices, within the unaligned kernel's bound
    lags = torch.tensor(SMALL["lags"], dtype=torch.int32).to(dev)
    got = ops.score_gram_lag(gr, ge, gm, tile, lags, D).cpu().numpy()
    r, c, lag = 1, 0, SMALL["lags"][1][0]
    rows = REF.gram_rows(refs[r, ..., D:L - D], np.stack([est[r, k, D + lag:L - D + lag] for k in range(2)]), mix[r, :, D:L - D], c, 0, tile)
    assert (np.abs(got[r, c, 0] - REF.gram_f64(rows)) <= (-(-tile // 256) + 16) * 2.0 ** -52 * REF.gram_abs(rows)).all()


def test_a_silent_target_gives_lag_zero_and_nan(dev, scorer):
    refs, est, mix, _ = (np.array(a) for a in AREF.case_inputs(SMALL))
    refs[0, 0] = 0.0                                                                   # recording 0: the target is digital silence
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, tile=SMALL["tile"], align=SMALL["D"])
    assert res["lag"][0].cpu().tolist() == [0, 0] and not bool(res["lag_track"][0].any()) and not bool(res["active"][0].any())
    assert bool(torch.isnan(res["whole"][0]).all()) and bool(torch.isnan(res["track"][0]).all())
    assert res["lag"][1].cpu().tolist() == SMALL["lags"][1] and bool(torch.isfinite(res["whole"][1]).all())


def test_aligned_score_makes_no_host_synchronisation(dev, scorer):
    """torch raises on any synchronising call while the mode is "error"; the twiddle table is on the device after the first call"""
    refs, est, mix, _ = AREF.case_inputs(SMALL)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    kw = dict(target=[0, 0], tile=SMALL["tile"], window=2, align=SMALL["D"])
    want = scorer.score(ge, gr, gm, **kw)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = scorer.score(ge, gr, gm, **kw)
        lone = scorer.score(ge, gr, gm, **dict(kw, target=[0, 1]))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same_result(res, want) and tuple(lone["lag"].shape) == (R, 2)


def test_refusals_launch_nothing(dev, scorer):
    from test_align_cpu import align_refusals
    lib = _lib.load()
    refs, est, mix, _ = AREF.case_inputs(SMALL)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    scorer.score(ge, gr, gm, align=300)
    n0 = lib.m2h_launch_count()
    for exc, pattern, kw in align_refusals():
        with pytest.raises(exc, match=pattern):
            scorer.score(ge, gr, gm, **kw)
    with pytest.raises(ValueError, match=r"L = 16385 samples; align = 8192 needs at least 2 \* 8192 \+ 2 = 16386"):
        scorer.score(ge[..., :16385], gr[..., :16385], gm[..., :16385], align=8192, tile=16384)
    assert lib.m2h_launch_count() == n0


def _write_wav(path, rate, data):
    from scipy.io import wavfile
    wavfile.write(path, rate, data)


def test_cli_align(dev, tmp_path):
    """score.py --align on int16 WAVs written from a shifted estimate: the printed lags, and the JSON's numbers against score_aligned_f64 on
    the WAV samples."""
    from scipy.io import wavfile
    refs, est, mix, _ = AREF.case_inputs(SMALL)
    D, lags, L = SMALL["D"], SMALL["lags"][0], SMALL["L"]
    q = lambda a: np.clip(np.rint(a.T * 32768.0), -32768, 32767).astype(np.int16)       # noqa: E731  [C, L] -> int16 [L, C]
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1", "ref2")}
    for k, v in (("est", est[0]), ("mix", mix[0]), ("ref0", refs[0, 0]), ("ref1", refs[0, 1]), ("ref2", refs[0, 2])):
        _write_wav(p[k], 16000, q(v))
    out_json = str(tmp_path / "scores.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"],
                          "--reference", p["ref1"], "--reference", p["ref2"], "--align", str(D), "--json", out_json],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout
    f = lambda path: (wavfile.read(path)[1].astype(np.float32) * np.float32(1.0 / 32768.0)).T          # noqa: E731
    want_whole, want_track = AREF.score_aligned_f64(np.stack([f(p["ref0"]), f(p["ref1"]), f(p["ref2"])]), f(p["est"]), f(p["mix"]), D, lags)
    got = json.load(open(out_json))
    assert got["align"] == D and got["lag"] == lags and got["region"] == [D, L - D] and got["windows"][0] == [D, D + 16000] and got["windows"][-1][1] == L - D
    assert len(got["lag_track"]) == 2 and all(len(row) == len(got["windows"]) for row in got["lag_track"])
    print("score.py --align JSON: whole %.3e dB, track %.3e dB of %.0e" % (REF.max_err(got["whole"], want_whole), REF.max_err(got["track"], want_track), REF.TOL_GPU))
    assert REF.max_err(got["whole"], want_whole) <= REF.TOL_GPU and REF.max_err(got["track"], want_track) <= REF.TOL_GPU
    lines = res.stdout.splitlines()
    assert any("samples [%d, %d) of the references and the mixture are scored" % (D, L - D) in ln for ln in lines), res.stdout
    for c, name in enumerate(("left", "right")):
        assert "%-8s lag %d samples (%.4f ms)" % (name, lags[c], lags[c] / 16.0) in lines, res.stdout
        row = [ln for ln in lines if ln.startswith("%-8s %-14s" % (name, "whole"))]
        assert len(row) == 1 and REF.max_err([float(v) for v in row[0][23:].split()], want_whole[c]) <= REF.TOL_GPU, res.stdout
    res = subprocess.run([sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"],
                          "--align", "9000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode != 0 and "align must be in 1 .. 8192 samples, got 9000" in res.stdout
