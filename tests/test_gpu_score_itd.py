"""The Scorer's broadband ITD on the GPU (m2h/audio/score.py "ITD", csrc/score_itd.hip): the tile sums, the GCC-PHAT functions, the picks
and the nine numbers against the float64 definition of tests/itd_ref.py within its bounds; bit-identical results whatever the call's
shape; special inputs; alignment at one lag for both ears; no side effect on any other number or kernel; no host synchronisation; the
refusals and the command line.

Measured on an MI355X (worst error / bound over the cases of test_sums_functions_and_picks_against_the_float64_definition): see
DESIGN.md §8.12."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import itd_ref as REF
from score_cases import _gpu, _same, _write_wav
from m2h import _lib, ops
from m2h.audio import score as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = REF.R
KEYS = ("itd_whole", "itd_track", "itd_gcc")
STEP = REF.US_PER_STEP


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scorer(dev):
    return SC.Scorer(dev)


@pytest.fixture(scope="module")
def tables(dev):
    return torch.from_numpy(SC.spectral_table()).to(dev), torch.from_numpy(SC.itd_table()).to(dev)


def stacked(L, D, shift, S):
    """the case of itd_ref as a batch: (refs [R, S, 2, L], est [R, 2, L], mix [R, 2, L]) float32, want: R dicts"""
    inputs, want = REF.case(L, D, shift, S)
    return [np.stack([inputs[r][k] for r in range(R)]) for k in range(3)], want


def check_nine(got, want, where):
    """the nine numbers [1 + M, 9] of one recording against the reference's dict: the ITDs equal where the margin exceeds 2 E and within one
    grid step elsewhere, the peaks within E, the errors and the improvement as they follow from the picks"""
    sure = want["margin"] > 2.0 * want["E"]
    d = np.abs(got[:, :3] - want["nine"][:, :3])
    assert (d[sure] == 0).all() and (d <= STEP).all(), (where, got[:, :3], want["nine"][:, :3])
    assert (np.abs(got[:, 6:] - want["nine"][:, 6:]) <= want["E"]).all(), where
    err, base = np.abs(got[:, 1] - got[:, 0]), np.abs(got[:, 2] - got[:, 0])
    assert (got[:, 3] == err).all() and (got[:, 4] == base).all() and (got[:, 5] == base - err).all(), where


@pytest.mark.parametrize("L,D,shift", REF.CASES)
@pytest.mark.parametrize("S", [2, 3])
def test_sums_functions_and_picks_against_the_float64_definition(dev, scorer, tables, L, D, shift, S):
    """16000: one tile; 16001: a tail tile of one sample; 40001: three tiles with a short tail; (40001, D = 300): aligned, the estimate 37
    samples late as a whole.  Both kernels twice: the same bits."""
    (refs, est, mix), want = stacked(L, D, shift, S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, align=D or None, itd=True)
    J, M = res["plan"]["J"], res["plan"]["M"]
    lag = None
    if D:
        lag = res["lag"]
        assert lag[:, 0].cpu().tolist() == [REF.left_lag(r, shift) for r in range(R)]
    sums = ops.score_itd(gr, ge, gm, 0, tables[0], lag, D)
    assert ops.last_kernel() == "score_itd" and sums.dtype == torch.float64 and tuple(sums.shape) == (R, J, 3, 256, 2)
    assert torch.equal(sums, ops.score_itd(gr, ge, gm, 0, tables[0], lag, D))
    whole = ops.score_windows(sums.view(R, 1, J, 1536), 1, J, 1)
    track = ops.score_windows(sums.view(R, 1, J, 1536), M, 1, 1)
    ws = torch.cat([whole, track], dim=2).view(R, 1 + M, 3, 256, 2)
    g = ops.itd_gcc(ws, tables[1], *SC.ITD_BINS)
    assert ops.last_kernel() == "itd_gcc" and g.dtype == torch.float64 and tuple(g.shape) == (R, 1 + M, 3, 257)
    assert torch.equal(g, ops.itd_gcc(ws, tables[1], *SC.ITD_BINS)) and torch.equal(g, res["itd_gcc"])
    nine = SC.itd_from_gcc(g, SC.itd_has_band(ws))
    assert _same(nine[:, 0], res["itd_whole"]) and _same(nine[:, 1:], res["itd_track"])
    assert tuple(res["itd_whole"].shape) == (R, 9) and tuple(res["itd_track"].shape) == (R, M, 9) and all(res[k].dtype == torch.float64 for k in KEYS)
    hs, hg, hn = sums.cpu().numpy(), g.cpu().numpy(), nine.cpu().numpy()
    for r in range(R):
        w = want[r]
        ws_, wg = REF.worst(hs[r], w["sums"], w["bound"][..., None]), float((np.abs(hg[r] - w["gcc"]) / w["E"][..., None]).max())
        print("score_itd S = %d, L = %d, D = %d, recording %d: sums worst error / bound %.3e; G worst error %.3e, worst error / E %.3e"
              % (S, L, D, r, ws_, np.abs(hg[r] - w["gcc"]).max(), wg))
        assert w["sums"].shape == (J, 3, 256, 2) and ws_ <= 1.0 and wg <= 1.0
        check_nine(hn[r], w, (S, L, D, r))
        assert hn[r, 0, 0] == 62.5 * REF.PLANTED[r][0][0] and hn[r, 0, 1] == 62.5 * min(REF.PLANTED[r][1], 16)       # as planted


def test_call_shape_changes_no_bit(dev, scorer):
    """each recording of a batch against its solo call, max_corr_bytes = 1 against the default, per-recording targets against solo calls,
    strided views against contiguous copies, odd L against 16-byte-aligned rows"""
    S, L = 3, 40001
    (refs, est, mix), _ = stacked(L, 0, 0, S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, window=2, hop=1, itd=True)
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), window=2, hop=1, itd=True)
        assert all(_same(solo[k][0], res[k][r]) for k in KEYS)
    one = SC.Scorer(dev, max_corr_bytes=1).score(ge, gr, gm, window=2, hop=1, itd=True)
    assert all(_same(one[k], res[k]) for k in KEYS)
    tg = [1, 2]
    per = SC.Scorer(dev, max_corr_bytes=1).score(ge, gr, gm, target=tg, window=2, hop=1, itd=True)
    both = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, itd=True)
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), target=tg[r], window=2, hop=1, itd=True)
        assert all(_same(solo[k][0], per[k][r]) and _same(solo[k][0], both[k][r]) for k in KEYS)
        assert float(both["itd_whole"][r, 0]) == 62.5 * REF.PLANTED[r][0][tg[r]]            # the other reference's delay
    images = torch.zeros((R + 1, S + 2, 2, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    strided = scorer.score(*views, window=2, hop=1, itd=True)
    assert all(_same(strided[k], res[k]) for k in KEYS)
    assert L % 4 == 1 and all(t.data_ptr() % 16 == 0 for t in (gr, ge, gm))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (3,), device=dev)], dim=-1)[..., :L]   # noqa: E731  (row stride L + 3 = 40004)
    aligned = scorer.score(pad(ge), pad(gr), pad(gm), window=2, hop=1, itd=True)
    assert all(_same(aligned[k], res[k]) for k in KEYS)


def test_special_inputs(dev, scorer, tables):
    """the same samples in both ears: CIM == 0 exactly, ITD 0 and peak 1 within E; a silent target: NaN itd, itd_err and itd_erri, no
    error, and the other recording unaffected"""
    S, L = 2, 16001
    (refs, est, mix), want = stacked(L, 0, 0, S)
    mono = np.ascontiguousarray(np.broadcast_to(est[:, :1], est.shape))
    gr, ge, gm = _gpu(dev, refs, mono, mix)
    sums = ops.score_itd(gr, ge, gm, 0, tables[0])
    assert bool((sums[:, :, 1, :, 1] == 0).all()) and bool((sums[:, :, 1, :, 0] >= 0).all())
    res = scorer.score(ge, gr, gm, itd=True)
    for r in range(R):
        o = REF.recording(refs[r], mono[r], mix[r])
        got = res["itd_gcc"][r, :, 1].cpu().numpy()
        assert (np.abs(got - o["gcc"][:, 1]) <= o["E"][:, 1:2]).all()
        assert (res["itd_whole"][r, 1] == 0) and bool((res["itd_track"][r, :, 1] == 0).all())
        assert abs(float(res["itd_whole"][r, 7]) - 1.0) <= o["E"][0, 1] and (np.abs(res["itd_track"][r, :, 7].cpu().numpy() - 1.0) <= o["E"][1:, 1]).all()
    silent = refs.copy()
    silent[0, 0] = 0.0
    gs, ge, gm = _gpu(dev, silent, est, mix)
    res, full = scorer.score(ge, gs, gm, itd=True), scorer.score(ge, gr, gm, itd=True)
    nan = torch.isnan(res["itd_whole"][0]).cpu().tolist()
    assert nan == [True, False, False, True, True, True, True, False, False]
    assert bool((torch.isnan(res["itd_track"][0]) == torch.isnan(res["itd_whole"][0])).all()) and bool((res["itd_gcc"][0, :, 0] == 0).all())
    assert all(_same(res[k][1], full[k][1]) for k in KEYS) and all(_same(res[k][0, ..., 1:3], full[k][0, ..., 1:3]) for k in ("itd_whole", "itd_track"))
    assert not bool(torch.isnan(full["itd_whole"]).any())
    check_nine(torch.cat([full["itd_whole"][1:2], full["itd_track"][1]]).cpu().numpy(), want[1], "next to a silent target")


def test_alignment_reads_both_ears_at_the_left_ears_lag(dev, scorer, tables):
    """align = 300 on an estimate that is 37 samples late as a whole: the sums are, bit for bit, those of slices cut by hand with BOTH
    ears at the left ear's lag, and the estimate keeps the ITD it has unshifted.  Each ear cut at its own lag -- the lag_right defect of
    the reference -- does not: aligned ear by ear the estimate takes on the target's delay."""
    L, D, shift, S = 40001, 300, 37, 2
    (refs, est, mix), want = stacked(L, D, shift, S)
    unshifted = REF.case(L, 0, 0, S)[1]
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, align=D, itd=True)
    lag = res["lag"].cpu().tolist()
    assert [l[0] for l in lag] == [REF.left_lag(r, shift) for r in range(R)], lag
    got = ops.score_itd(gr, ge, gm, 0, tables[0], res["lag"], D)
    for r in range(R):
        l0, l1 = lag[r]
        cut = (ge[r:r + 1, :, D + l0:L - D + l0], gr[r:r + 1, ..., D:L - D], gm[r:r + 1, :, D:L - D])
        assert torch.equal(got[r:r + 1], ops.score_itd(cut[1], cut[0], cut[2], 0, tables[0]))
        by_hand = scorer.score(*cut, itd=True)
        assert all(_same(res[k][r], by_hand[k][0]) for k in KEYS)
        assert float(res["itd_whole"][r, 1]) == want[r]["nine"][0, 1] == unshifted[r]["nine"][0, 1] == 62.5 * min(REF.PLANTED[r][1], 16)
        assert REF.worst(got[r].cpu().numpy(), want[r]["sums"], want[r]["bound"][..., None]) <= 1.0
        per_ear = torch.stack([ge[r, 0, D + l0:L - D + l0], ge[r, 1, D + l1:L - D + l1]])[None]
        own = scorer.score(per_ear, cut[1], cut[2], itd=True)
        defect = REF.recording(refs[r], est[r], mix[r], 0, l0, D, lag_right=l1)
        check_nine(torch.cat([own["itd_whole"], own["itd_track"][0]]).cpu().numpy(), defect, ("lag_right", r))
        a, b = float(res["itd_whole"][r, 1]), float(own["itd_whole"][0, 1])
        print("recording %d: the estimate's ITD %.4f us at one lag, %.4f us with each ear at its own lag (the target's: %.4f us)"
              % (r, a, b, float(res["itd_whole"][r, 0])))
        assert abs(b - a) > 2 * STEP and abs(b - float(res["itd_whole"][r, 0])) <= 62.5          # (each lag is rounded to a sample)
        miss = np.abs(defect["sums"] - want[r]["sums"]) / want[r]["bound"][..., None]
        assert miss.max() > 1.0


def test_itd_changes_no_other_number_and_no_other_kernel(dev, scorer, tables):
    S, L = 3, 40001
    (refs, est, mix), _ = stacked(L, 0, 0, S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    spat0, spec0 = ops.score_spatial(gr, ge, gm, 0, tables[0]), ops.score_spectral(gr, ge, gm, 0, tables[0])
    kw = dict(window=2, hop=1, align=16, spectral=True, spatial=True, stoi=True, bss=8)
    plain = scorer.score(ge, gr, gm, **kw)
    res = scorer.score(ge, gr, gm, itd=True, **kw)
    off = scorer.score(ge, gr, gm, itd=False, **kw)
    assert not [k for k in list(plain) + list(off) if k.startswith("itd")] and sorted(set(res) - set(plain)) == sorted(KEYS)
    for k in plain:
        if k != "plan":
            assert _same(res[k], plain[k]) and _same(off[k], plain[k]), k
    assert res["plan"] == plain["plan"] and {"lag", "lag_track", "spectral_track", "spatial_cues", "stoi_frames", "bss_track"} <= set(plain)
    alone = scorer.score(ge, gr, gm, window=2, hop=1, align=16, itd=True)
    assert all(_same(alone[k], res[k]) for k in KEYS)
    # the two kernels that share the transform: the same bits after this change's kernel has run as before it, on one input
    assert torch.equal(ops.score_spatial(gr, ge, gm, 0, tables[0]), spat0) and torch.equal(ops.score_spectral(gr, ge, gm, 0, tables[0]), spec0)
    # and the cross terms of the spatial kernel are this kernel's, band by band: 16 bins added (another order of additions: to rounding)
    sums = ops.score_itd(gr, ge, gm, 0, tables[0])
    bands = sums.view(R, -1, 3, 16, 16, 2).sum(dim=4)
    scale = spat0[..., :16, :2].sum(dim=-1, keepdim=True)                                # PL + PR of the band: at least twice the sum of the |terms| added
    assert bool(((bands - spat0[..., :16, 2:]).abs() <= 1e-12 * scale).all())


def test_itd_path_makes_no_host_synchronisation(dev, scorer):
    """torch raises on any synchronising call (a copy from pageable host memory, .item(), a boolean mask) while the mode is "error"."""
    (refs, est, mix), _ = stacked(40001, 0, 0, 3)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    small = SC.Scorer(dev, max_corr_bytes=1)
    want = scorer.score(ge, gr, gm, target=[0, 1], window=2, itd=True)
    aligned = small.score(ge, gr, gm, target=[0, 1], window=2, align=16, itd=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = scorer.score(ge, gr, gm, target=[0, 1], window=2, itd=True)
        res16 = small.score(ge, gr, gm, target=[0, 1], window=2, align=16, itd=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(_same(res[k], want[k]) for k in KEYS) and all(_same(res16[k], aligned[k]) for k in KEYS)


def test_refusals_launch_nothing(dev, scorer):
    lib = _lib.load()
    z = lambda *shape: torch.zeros(shape, device=dev)                                   # noqa: E731
    est, refs, mix = z(2, 2, 50), z(2, 3, 2, 50), z(2, 2, 50)
    torch.cuda.synchronize()
    n0 = lib.m2h_launch_count()
    with pytest.raises(ValueError, match="itd=True .* needs C = 2 channels, got C = 1"):
        scorer.score(z(2, 50), z(2, 3, 50), mix, itd=True)
    with pytest.raises(ValueError, match="itd=True needs tile = 16000 .*got 8000"):
        scorer.score(est, refs, mix, itd=True, tile=8000)
    for bad in (1, None, "yes"):
        with pytest.raises(TypeError, match="itd must be a bool, got %r" % (bad,)):
            scorer.score(est, refs, mix, itd=bad)
    with pytest.raises(RuntimeError, match="score_itd: C = 1 channels"):
        ops.score_itd(z(2, 3, 1, 50), z(2, 1, 50), mix, 0, torch.from_numpy(SC.spectral_table()).to(dev))
    with pytest.raises(RuntimeError, match="k_lo = 6 .. k_hi = 257"):
        ops.itd_gcc(torch.zeros((2, 256, 2), device=dev, dtype=torch.float64), torch.from_numpy(SC.itd_table()).to(dev), 6, 257)
    with pytest.raises(RuntimeError, match=r"itd_gcc: sums must be \[..., 256, 2\]"):
        ops.itd_gcc(torch.zeros((2, 255, 2), device=dev, dtype=torch.float64), torch.from_numpy(SC.itd_table()).to(dev), 6, 256)
    assert lib.m2h_launch_count() == n0


def test_cli_itd_rows_and_json(dev, tmp_path):
    """score.py --itd --json on int16 two-channel WAVs of a planted pair: the printed and the JSON ITDs are as planted, every number
    matches the float64 definition on the WAV's samples, the rows are the JSON's; without the flag none of the new keys and rows appear
    and everything else is byte for byte the same; mono files are refused."""
    S, L = 2, 40001
    refs, est, mix = REF.planted(0, L, S)
    q = lambda a: np.clip(np.rint(np.asarray(a, np.float64) * 32768.0), -32768, 32767).astype(np.int16)      # noqa: E731
    back = lambda a: a.astype(np.float32) * np.float32(1.0 / 32768.0)                                        # noqa: E731
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1", "mono")}
    for k, v in (("est", est), ("mix", mix), ("ref0", refs[0]), ("ref1", refs[1])):
        _write_wav(p[k], np.ascontiguousarray(q(v).T))
    _write_wav(p["mono"], q(est[0]))
    out_json = str(tmp_path / "scores.json")
    cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"], "--reference", p["ref1"],
           "--json", out_json]
    run = lambda c: subprocess.run(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)   # noqa: E731
    res = run(cmd + ["--itd"])
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    want = REF.recording(back(q(refs)), back(q(est)), back(q(mix)))
    J = want["sums"].shape[0]
    assert (want["margin"] > 2.0 * want["E"]).all()
    assert got["itd_metrics"] == list(REF.ORDER) and np.array(got["itd_track"]).shape == (J, 9) and np.array(got["itd_gcc"]).shape == (1 + J, 3, 257)
    assert got["itd_whole"][:2] == [62.5 * REF.PLANTED[0][0][0], 62.5 * REF.PLANTED[0][1]] == [1000.0, 156.25]
    check_nine(np.array([got["itd_whole"]] + got["itd_track"]), want, "cli")
    assert (np.abs(np.array(got["itd_gcc"]) - want["gcc"]) <= want["E"][..., None]).all()
    assert np.allclose(got["itd_track_mean"], np.mean(got["itd_track"], axis=0), rtol=1e-12, atol=0)
    assert np.allclose(got["itd_track_median"], np.median(got["itd_track"], axis=0), rtol=1e-12, atol=0)
    lines = res.stdout.splitlines()
    for label, key in (("itd whole", "itd_whole"), ("itd window mean", "itd_track_mean"), ("itd window median", "itd_track_median")):
        row = [ln for ln in lines if ln.startswith("%-8s %-23s" % ("binaural", label))]
        assert len(row) == 1, res.stdout
        assert np.allclose([float(v) for v in row[0][32:].split()], got[key], rtol=1e-11, atol=0), (label, row[0])
    assert [float(v) for v in [ln for ln in lines if ln.startswith("%-8s %-23s" % ("binaural", "itd whole"))][0][32:].split()][:2] == [1000.0, 156.25]
    with_flag, with_lines = got, lines
    res = run(cmd)
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    assert not [k for k in got if k.startswith("itd")]
    assert json.dumps({k: v for k, v in with_flag.items() if not k.startswith("itd")}) == json.dumps(got)
    assert res.stdout.splitlines() == [ln for ln in with_lines if not ln.startswith(("itd us", "binaural"))]
    mono_cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["mono"], "--mixture", p["mix"], "--reference", p["mono"], "--itd"]
    res = run(mono_cmd)
    assert res.returncode != 0 and "two channels are needed" in res.stdout, res.stdout
