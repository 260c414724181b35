"""BSS-eval SDR / SIR / SAR of the Scorer on the GPU (m2h/audio/score.py "BSS", csrc/score_bss.hip) against tests/bss_ref.py: the lagged
correlations within the element-wise bound of an fp64 sum of exact products, the projection kernel on the kernel's own filters within the
textbook bound, Scorer.score(..., bss=T) end to end within TOL_BSS, its bit-identical properties (two runs, batch against solo, strided
views, alignment against hand-cut slices, every other key untouched), silent references, the filtered estimate, the command line, and what
the path does under torch's synchronisation warnings.

Measured on an MI355X: see DESIGN.md §8.11."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import bss_ref as B
import score_ref
from score_cases import R, _gpu, _same, _target, _write_wav, recordings, targets
from m2h import ops
from m2h.audio import score as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("bss_whole", "bss_track")
CONFIGS = [(1, 1), (2, 1)]                                   # (window, hop) in tiles
KERNEL_CASES = [(3301, 1500, 512, 3, 2, 0), (530, 97, 37, 2, 1, 0), (530, 97, 37, 2, 1, 16), (1100, 1100, 5, 1, 2, 0)]      # (L, tile, T, S, C, D)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scorer(dev):
    return SC.Scorer(dev)


def batch(S, C, L, which="plain"):
    """R recordings of score_ref.inputs, or with the filtered estimate: refs [R, S, C, L], est [R, C, L], mix [R, 2, L]"""
    tg = targets(S)

    def one(r):
        refs, est, mix = score_ref.inputs(S, L, 31 + 50 * r, C)
        if which == "filtered":                              # the target of recording r through the FIR
            order = [tg[r]] + [i for i in range(S) if i != tg[r]]
            est = B.filtered_estimate(refs[order], mix, 7 + r)
        return refs, est, mix
    return recordings(("bss", S, C, L, which), one)


def reference(case, which):
    """bss_ref route a of every recording of a case, for every window setting of CONFIGS: [(whole [R, C, 9], track [R, C, M, 9])]"""
    L, tile, T, S, C = case
    refs, est, mix = batch(S, C, L, which)
    tg = targets(S)
    per = recordings(("bss ref", case, which), lambda r: tuple(a for res in B.bss_direct(refs[r], est[r], mix[r], tg[r], tile, CONFIGS, None, T) for a in res))
    return [(per[2 * k], per[2 * k + 1]) for k in range(len(CONFIGS))]


def lag_table(dev, C, D):
    """(lag [R, C] int32 on the device, the same as lists), some beyond [-D, D]: the kernels clamp"""
    if not D:
        return None, [[0] * C] * R
    lags = [[5, -D - 9][:C], [-3, D][:C]]
    return torch.tensor(lags, dtype=torch.int32).to(dev), [[max(-D, min(D, v)) for v in row] for row in lags]


@pytest.mark.parametrize("L,tile,T,S,C,D", KERNEL_CASES)
def test_corr_is_within_the_bound_of_an_fp64_sum_of_exact_products(dev, L, tile, T, S, C, D):
    """every entry of every tile against a longdouble sum of the exact products: |err| <= n 2^-53 sum |a b|"""
    refs, est, mix = batch(S, C, L)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    lag, lags = lag_table(dev, C, D)
    got = ops.bss_corr(gr, ge, gm, tile, T, lag, D)
    assert ops.last_kernel() == "bss_corr" and tuple(got.shape) == (R, C, -(-(L - 2 * D) // tile), S, S + 2, T)
    got = got.cpu().numpy()
    worst = 0.0
    for r in range(R):
        for c in range(C):
            s, x, b = B.signals(refs[r], est[r], mix[r], c, D, lags[r][c])
            want, mag, n = B.corr_tiles_exact(s, list(s) + [x, b], T, tile)
            bound = n[:, None, None, None] * B.U * mag
            err = np.abs(got[r, c] - want)
            assert (err <= bound).all(), (r, c, float((err / np.maximum(bound, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("bss_corr %s: worst error / bound %.3e" % ((L, tile, T, S, C, D), worst))
    assert _same(torch.from_numpy(got), ops.bss_corr(gr, ge, gm, tile, T, lag, D).cpu())


@pytest.mark.parametrize("L,tile,T,S,C,D", KERNEL_CASES)
def test_project_on_the_kernels_own_filters(dev, L, tile, T, S, C, D):
    """the ten sums of every tile against numpy float64 on the same filters, within twice the bound of tests/bss_ref.py"""
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    lag, lags = lag_table(dev, C, D)
    J = -(-(L - 2 * D) // tile)
    co = ops.bss_corr(gr, ge, gm, tile, T, lag, D)
    whole = ops.score_windows(co.view(R, C, J, S * (S + 2) * T), 1, J, 1).view(R, C, S, S + 2, T)
    h, ok = SC.bss_filters(whole, tg)
    assert bool(ok.all())
    got = ops.bss_project(gr, ge, gm, _target(dev, tg), h, tile, lag, D)
    assert ops.last_kernel() == "bss_project" and tuple(got.shape) == (R, C, J, 10)
    worst = 0.0
    for r in range(R):
        for c in range(C):
            s, x, b = B.signals(refs[r], est[r], mix[r], c, D, lags[r][c])
            want, bound = B.project_tiles(s, x, b, h[r, c].cpu().numpy(), tg[r], tile)
            err = np.abs(got[r, c].cpu().numpy() - want)
            assert (err <= 2 * bound).all(), (r, c, float((err / (2 * bound)).max()))
            worst = max(worst, float((err / (2 * bound)).max()))
    print("bss_project %s: worst error / (2 bound) %.3e" % ((L, tile, T, S, C, D), worst))
    assert _same(got, ops.bss_project(gr, ge, gm, _target(dev, tg), h, tile, lag, D))


@pytest.mark.parametrize("case", B.CASES)
def test_the_nine_numbers_are_within_tol_bss(dev, scorer, case):
    L, tile, T, S, C = case
    tg = targets(S)
    for which in (("plain", "filtered") if L >= 300 else ("plain",)):
        refs, est, mix = batch(S, C, L, which)
        gr, ge, gm = _gpu(dev, refs, est, mix)
        gr, ge = (gr, ge) if C == 2 else (gr[:, :, 0], ge[:, 0])       # C = 1: the three- and two-dimensional forms
        for (window, hop), (whole, track) in zip(CONFIGS, reference(case, which)):
            res = scorer.score(ge, gr, gm, target=tg, tile=tile, window=window, hop=hop, bss=T)
            gw, gt = res["bss_whole"].cpu().numpy(), res["bss_track"].cpu().numpy()
            assert gw.shape == whole.shape == (R, C, 9) and gt.shape == track.shape == (R, C, res["plan"]["M"], 9)
            assert np.array_equal(np.isnan(gw), np.isnan(whole)) and np.array_equal(np.isnan(gt), np.isnan(track))
            ew, et = B.max_err(gw, whole), B.max_err(gt, track)
            print("bss %-28s %-8s window %d / %d: whole %.3e dB, track %.3e dB (TOL_BSS %.2e)" % (case, which, window, hop, ew, et, B.TOL_BSS))
            assert ew <= B.TOL_BSS and et <= B.TOL_BSS, (case, which, window, ew, et)


def test_bit_identity_batch_strides_and_the_other_keys(dev, scorer):
    S, C, L, T = 3, 2, 16001, 512
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, bss=T)
    again = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, bss=T)
    assert all(_same(res[k], again[k]) for k in KEYS)
    for r in range(R):                                        # each recording of the batch equals its solo call
        solo = scorer.score(ge[r:r + 1], gr[r:r + 1], gm[r:r + 1], target=tg[r], window=2, hop=1, bss=T)
        assert all(_same(solo[k][0], res[k][r]) for k in KEYS), r
    small = SC.Scorer(dev, max_corr_bytes=1)                  # one recording per group of the correlation buffer
    assert all(_same(small.score(ge, gr, gm, target=tg, window=2, hop=1, bss=T)[k], res[k]) for k in KEYS)
    # strided views inside larger buffers at odd element offsets
    images = torch.zeros((R + 1, S + 2, C, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    strided = scorer.score(*views, target=tg, window=2, hop=1, bss=T)
    assert all(_same(strided[k], res[k]) for k in KEYS)
    # every other key with and without bss, composed with align, spectral, spatial and stoi
    for kw in (dict(), dict(spectral=True, spatial=True, stoi=True), dict(align=16, spectral=True, spatial=True, stoi=True)):
        without = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, **kw)
        with_bss = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, bss=T, **kw)
        assert not any(k in without for k in KEYS) and set(with_bss) == set(without) | set(KEYS)
        for k, v in without.items():
            assert with_bss[k] == v if k == "plan" else (_same(with_bss[k], v) if v.dtype.is_floating_point else torch.equal(with_bss[k], v)), (kw, k)
        if "align" not in kw:
            assert all(_same(with_bss[k], res[k]) for k in KEYS)


def test_alignment_equals_hand_cut_slices(dev, scorer):
    """align=64 on an estimate that is the target late by 37 samples in the left ear and 40 in the right: the same bits as slices cut by hand
    at those lags and scored without align"""
    D, lags, S, C, T = 64, [37, 40], 3, 2, 512
    L = 2 * D + 16001
    refs, _, mix = batch(S, C, L)
    tg = targets(S)
    rng = np.random.default_rng(9)
    est = np.zeros((R, C, L), np.float32)
    for r in range(R):
        for c in range(C):
            est[r, c, lags[c]:] = refs[r, tg[r], c, :L - lags[c]]
    est += (0.01 * rng.standard_normal(est.shape)).astype(np.float32)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, align=D, bss=T)
    assert res["lag"].cpu().tolist() == [lags] * R
    cut_est = torch.stack([ge[:, c, D + lags[c]:L - D + lags[c]] for c in range(C)], dim=1)
    cut = scorer.score(cut_est, gr[..., D:L - D], gm[..., D:L - D], target=tg, bss=T)
    assert all(_same(res[k], cut[k]) for k in KEYS)
    # the target's power is about 0.02 * 1.125 + 0.05^2 and the added noise's 0.01^2: 24 dB once the delay is absorbed
    assert res["plan"]["J"] == 2 and tuple(res["bss_track"].shape) == (R, C, 2, 9) and bool((res["bss_whole"][..., 0] > 20).all())
    want = [B.bss_direct(refs[r], est[r], mix[r], tg[r], 16000, 1, 1, T, D=D, lags_=lags) for r in range(R)]
    assert B.max_err(res["bss_whole"].cpu().numpy(), np.stack([w[0] for w in want])) <= B.TOL_BSS
    assert B.max_err(res["bss_track"].cpu().numpy(), np.stack([w[1] for w in want])) <= B.TOL_BSS


def test_silent_references(dev, scorer):
    """a silent interferer is left out of the projection; a silent target gives NaN for its recording and leaves the other one alone"""
    S, C, L, T, tile = 3, 1, 2000, 128, 700
    refs, est, mix = batch(S, C, L)
    refs = refs.copy()
    refs[:, 0] = 0.0                                          # reference 0: an interferer of both recordings (targets 1 and 2)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=[1, 2], tile=tile, bss=T)
    for r, t in enumerate([1, 2]):
        whole, track = B.bss_direct(refs[r, 1:], est[r], mix[r], t - 1, tile, 1, 1, T)         # the call without the silent reference
        assert B.max_err(res["bss_whole"][r].cpu().numpy(), whole) <= B.TOL_BSS and B.max_err(res["bss_track"][r].cpu().numpy(), track) <= B.TOL_BSS
    quiet = scorer.score(ge, gr, gm, target=[0, 2], tile=tile, bss=T)                          # recording 0: a silent target
    assert bool(torch.isnan(quiet["bss_whole"][0]).all()) and bool(torch.isnan(quiet["bss_track"][0]).all())
    assert all(_same(quiet[k][1], res[k][1]) for k in KEYS)


def test_the_filtered_estimate_misses_its_si_sdr_by_more_than_10_db(dev, scorer):
    S, C, L = 3, 2, 16001
    refs, est, mix = batch(S, C, L, "filtered")
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=targets(S), bss=512)
    si_sdr, sdr = res["whole"][..., 0].cpu().numpy(), res["bss_whole"][..., 0].cpu().numpy()
    print("filtered estimate: si_sdr %s dB, bss sdr %s dB" % (np.round(si_sdr, 2).tolist(), np.round(sdr, 2).tolist()))
    assert (sdr - si_sdr > 10).all()
    s = SC.summarize(res)
    assert s["bss_metrics"] == list(SC.BSS_ORDER) and np.allclose(s["bss_whole"], res["bss_whole"].cpu().numpy(), rtol=0, atol=0)
    active, track = res["active"].cpu().numpy(), res["bss_track"].cpu().numpy()
    assert active.tolist() == [[[True, False]] * C] * R                                  # (the second window is one sample: no centred energy)
    assert np.allclose(s["bss_track_mean"], track[:, :, 0], rtol=1e-12, atol=0) and np.allclose(s["bss_track_median"], track[:, :, 0], rtol=1e-12, atol=0)


def test_the_bss_path_under_synchronisation_warnings(dev, scorer):
    """The Scorer's own code makes no host synchronisation; whether torch's factorisation does is observed here and recorded in DESIGN.md
    8.11, not asserted: the call runs under set_sync_debug_mode("warn"), prints what warned and must return the same bits."""
    refs, est, mix = batch(3, 2, 16001)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    want = scorer.score(ge, gr, gm, target=[0, 1], bss=64)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            res = scorer.score(ge, gr, gm, target=[0, 1], bss=64)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for w in seen:
        print("bss under sync warnings: %s:%d: %s" % (w.filename, w.lineno, str(w.message).splitlines()[0]))
    print("bss under sync warnings: %d warning(s)" % len(seen))
    assert all(_same(res[k], want[k]) for k in KEYS)
    assert not [w for w in seen if os.path.basename(w.filename) == "ops.py"]        # no m2h op synchronises


def test_argument_errors_launch_nothing(dev, scorer):
    from m2h import _lib
    lib = _lib.load()
    z = lambda *shape, **kw: torch.zeros(shape, device=dev, **kw)   # noqa: E731
    ok = dict(estimate=z(R, 2000), references=z(R, 3, 2000), mixture=z(R, 2, 2000))
    n0 = lib.m2h_launch_count()
    for bad, exc in ((True, TypeError), (4.0, TypeError), (0, ValueError), (513, ValueError), (512, None)):
        if exc is None:
            exc, ok = ValueError, dict(estimate=z(R, 1535), references=z(R, 3, 1535), mixture=z(R, 2, 1535))
        with pytest.raises(exc, match="bss"):
            scorer.score(bss=bad, **ok)
    sig = (z(R, 3, 1, 50), z(R, 1, 50), z(R, 2, 50))
    with pytest.raises(RuntimeError, match="T = 513 in 1 .. 512"):
        ops.bss_corr(*sig, 16, 513)
    with pytest.raises(RuntimeError, match="with a lag"):
        ops.bss_corr(*sig, 16, 4, lag=None, D=4)
    with pytest.raises(RuntimeError, match=r"h must be \[R, C, 2, S \+ 1, T\]"):
        ops.bss_project(*sig, 0, z(R, 1, 2, 3, 4, dtype=torch.float64), 16)
    with pytest.raises(RuntimeError, match="expected torch.float64"):
        ops.bss_project(*sig, 0, z(R, 1, 2, 4, 4), 16)
    assert lib.m2h_launch_count() == n0
    assert bool(torch.isnan(scorer.score(bss=8, **ok)["bss_whole"]).all())               # digital silence: a silent target


def test_cli_bss_rows_and_json(dev, tmp_path):
    """score.py --bss --json on float32 WAVs of 20001 samples against bss_ref; without the flag no bss key or row, the rest byte-equal."""
    S, C, L = 2, 2, 20001
    refs, est, mix = score_ref.inputs(S, L, 77, C)
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1")}
    for k, v in (("est", est), ("mix", mix), ("ref0", refs[0]), ("ref1", refs[1])):
        _write_wav(p[k], np.ascontiguousarray(v.T))
    out_json = str(tmp_path / "scores.json")
    cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"], "--reference", p["ref1"],
           "--json", out_json]
    run = lambda c: subprocess.run(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)   # noqa: E731
    res = run(cmd + ["--bss"])
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    whole, track = B.bss_direct(refs, est, mix, 0, 16000, 1, 1, 512)
    assert got["bss_metrics"] == list(B.BSS_ORDER) and got["bss_taps"] == 512
    assert B.max_err(np.array(got["bss_whole"]), whole) <= B.TOL_BSS and B.max_err(np.array(got["bss_track"]), track) <= B.TOL_BSS
    assert np.allclose(got["bss_track_mean"], track.mean(axis=1), rtol=1e-9, atol=0)
    lines = res.stdout.splitlines()
    for c, name in enumerate(("left", "right")):
        for label, key in (("bss whole", "bss_whole"), ("bss window mean", "bss_track_mean"), ("bss window median", "bss_track_median")):
            row = [ln for ln in lines if ln.startswith("%-8s %-23s" % (name, label))]
            assert len(row) == 1, res.stdout
            assert np.allclose([float(v) for v in row[0][32:].split()], got[key][c], rtol=1e-11, atol=0), (name, label, row[0])
    with_flag, with_lines = got, lines
    res = run(cmd)
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    assert not [k for k in got if k.startswith("bss")]
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith("bss") or "bss w" in ln]
    assert json.dumps({k: v for k, v in with_flag.items() if not k.startswith("bss")}) == json.dumps(got)
    assert [ln for ln in with_lines if not (ln.startswith("bss") or "bss w" in ln)] == res.stdout.splitlines()
