"""The Scorer's interaural cues on the GPU (m2h/audio/score.py "Spatial", csrc/score_spatial.hip): the band sums of every tile against the
float64 definition of tests/spatial_ref.py within its bound, the cross-check against m2h_score_spectral's energies,
Scorer.score(..., spatial=True) and its bit-identical properties, alignment at one lag for both ears, no host synchronisation, the
Auralizer -> Separator -> Scorer scenario and the command line.

Measured on an MI355X (worst error / bound over the cases of test_tile_sums_against_the_float64_definition): see DESIGN.md §8.9."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spatial_ref as REF
import spectral_ref as SR
from score_cases import LMAX, R, _gpu, _same, _target, _write_wav, batch, recordings, targets
from m2h import ops
from m2h.audio import score as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("spatial_whole", "spatial_track", "spatial_cues")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scorer(dev):
    return SC.Scorer(dev)


@pytest.fixture(scope="module")
def table(dev):
    return torch.from_numpy(SC.spectral_table()).to(dev)


def click_batch():
    return recordings("click pairs", lambda r: REF.click_pairs(seed=r))


def reference(key, refs, est, mix, tg, lag=None, D=0):
    """(sums [R, J, 3, 32, 4], bound [R, J, 3, 32, 4]) float64 of a batch; computed once per key"""
    return recordings(("spatial", key), lambda r: REF.recording_sums(refs[r], est[r], mix[r], tg[r], 0 if lag is None else lag[r], D))


@pytest.mark.parametrize("S,L", [(S, L) for S in (1, 3) for L in (1, 5, 700, 15999, 16000, 16001, 40001)] + [(1, "clicks")])
def test_tile_sums_against_the_float64_definition(dev, table, S, L):
    """L = 1 and 16001 are the smallest shapes at which zero extension, reflection and the second tile can go wrong; the clicks show frame
    placement, which noise-like inputs hide."""
    if L == "clicks":
        refs, est, mix = click_batch()
    else:
        refs, est, mix = (a[..., :L] for a in batch(S))
    tg = targets(S)
    want, bound = reference((S, L), refs, est, mix, tg)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    got = ops.score_spatial(gr, ge, gm, _target(dev, tg), table)
    torch.cuda.synchronize()
    assert ops.last_kernel() == "score_spatial" and got.dtype == torch.float64 and tuple(got.shape) == want.shape
    w = REF.worst(got.cpu().numpy(), want, bound)
    print("score_spatial S = %d, L = %s: worst error / bound %.3e" % (S, L, w))
    assert w <= 1.0


def test_band_energies_add_up_to_the_spectral_kernels(dev, table):
    """sum over the bands of PL and PR of G, E, B against m2h_score_spectral's sums 0, 1, 2 of the two ears, within the two bounds added"""
    S = 3
    refs, est, mix = batch(S)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    spat = ops.score_spatial(gr, ge, gm, _target(dev, tg), table).cpu().numpy()         # [R, J, 3, 32, 4]
    spec = ops.score_spectral(gr, ge, gm, _target(dev, tg), table).cpu().numpy()        # [R, 2, J, 7]
    _, bound = reference((S, LMAX), refs, est, mix, tg)
    sbound = np.stack([SR.recording_sums(refs[r], est[r], mix[r], tg[r])[1] for r in range(R)])
    worst = 0.0
    for c in range(2):
        d = np.abs(spat[..., c].sum(axis=-1) - spec[:, c, :, :3])                       # [R, J, 3]
        tol = bound[..., c].sum(axis=-1) + sbound[:, c, :, :3]
        worst = max(worst, float((d / tol).max()))
    print("band energies against score_spectral: worst difference / (bound + bound) %.3e" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("window,hop", [(1, 1), (2, 1)])
def test_scorer_spatial_is_spatial_from_sums_of_the_windowed_sums(dev, scorer, table, window, hop):
    S = 3
    refs, est, mix = batch(S)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, window=window, hop=hop, spectral=True, spatial=True)
    plain = scorer.score(ge, gr, gm, target=tg, window=window, hop=hop)
    spec = scorer.score(ge, gr, gm, target=tg, window=window, hop=hop, spectral=True)
    J, M = res["plan"]["J"], res["plan"]["M"]
    assert not [k for k in list(plain) + list(spec) if k.startswith("spatial")]
    assert tuple(res["spatial_whole"].shape) == (R, 9) and tuple(res["spatial_track"].shape) == (R, M, 9)
    assert tuple(res["spatial_cues"].shape) == (R, M, 3, 32, 3) and all(res[k].dtype == torch.float64 for k in KEYS)
    for k in ("whole", "track"):                                                        # the eleven BSS numbers do not move by a bit
        assert _same(res[k], plain[k])
    assert bool(torch.equal(res["active"], plain["active"]))
    for k in ("spectral_whole", "spectral_track"):                                      # nor do the spectral ones
        assert _same(res[k], spec[k])
    tiles = ops.score_spatial(gr, ge, gm, _target(dev, tg), table).view(R, 1, J, 384)
    whole = SC.spatial_from_sums(ops.score_windows(tiles, 1, J, 1).view(R, 1, 3, 32, 4))
    track = SC.spatial_from_sums(ops.score_windows(tiles, M, window, hop).view(R, M, 3, 32, 4))
    assert _same(res["spatial_whole"], whole[0][:, 0]) and _same(res["spatial_track"], track[0]) and _same(res["spatial_cues"], track[1])
    # and the numbers themselves against the definition, within the bound that follows from the sums'
    want, bound = reference((S, LMAX), refs, est, mix, tg)
    for r in range(R):
        ws, wb = REF.window_sums(want[r], window, hop), REF.window_sums(bound[r], window, hop)
        d = np.abs(res["spatial_track"][r].cpu().numpy() - REF.metrics(ws))
        tol = REF.metrics_bound(ws, wb)
        assert np.isfinite(tol).all() and (d <= tol).all(), (r, d, tol)


def test_batch_slices_strides_and_alignment_are_bit_identical(dev, scorer):
    S, L = 3, LMAX
    refs, est, mix = batch(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, window=2, hop=1, spatial=True)
    one = scorer.score(ge, gr, gm, spatial=True)
    # each recording of the batch against its solo score
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), window=2, hop=1, spatial=True)
        assert all(_same(solo[k][0], res[k][r]) for k in KEYS)
    # track[m] against that slice scored as a whole (slices start at tile multiples)
    for plan_res in (res, one):
        for m, (t0, t1) in enumerate(plan_res["plan"]["samples"]):
            alone = scorer.score(ge[..., t0:t1], gr[..., t0:t1], gm[..., t0:t1], window=2, spatial=True)
            assert _same(alone["spatial_whole"], plan_res["spatial_track"][:, m]), (m, t0, t1)
            assert _same(alone["spatial_cues"][:, 0], plan_res["spatial_cues"][:, m]), (m, t0, t1)
    # strided views inside larger buffers against contiguous copies
    images = torch.zeros((R + 1, S + 2, 2, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    strided = scorer.score(*views, window=2, hop=1, spatial=True)
    assert all(_same(strided[k], res[k]) for k in KEYS)
    # odd L puts every second row of the contiguous tensors at an odd element offset; the same data in rows that are all 16-byte aligned
    assert L % 4 == 1 and all(t.data_ptr() % 16 == 0 for t in (gr, ge, gm))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (3,), device=dev)], dim=-1)[..., :L]   # noqa: E731  (row stride L + 3 = 40004)
    aligned = scorer.score(pad(ge), pad(gr), pad(gm), window=2, hop=1, spatial=True)
    assert all(_same(aligned[k], res[k]) for k in KEYS)


def test_alignment_reads_both_ears_at_the_left_ears_lag(dev, scorer, table):
    """align=64 on an estimate whose ears are the target's delayed by 37 and 40 samples plus noise: the lags found are 37 and 40, the
    spatial sums are, bit for bit, those of slices cut by hand with BOTH ears at 37 and passed without align, and the 3 samples of
    interaural delay the estimate added show in ipd_err; cut per ear they would vanish."""
    D, lags = 64, (37, 40)
    L = 2 * D + 16001
    rng = np.random.default_rng(9)
    refs = np.stack([REF.binaural(seed=20 + r, L=L)[0] for r in range(R)])               # [R, 1, 2, L]
    mix = np.stack([REF.binaural(seed=20 + r, L=L)[2] for r in range(R)])
    est = np.zeros((R, 2, L), np.float32)
    for c in range(2):
        est[:, c, lags[c]:] = refs[:, 0, c, :L - lags[c]]
    est += (0.001 * rng.standard_normal(est.shape)).astype(np.float32)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, align=D, spatial=True)
    assert res["lag"].cpu().tolist() == [list(lags)] * R
    assert res["plan"]["J"] == 2 and tuple(res["spatial_track"].shape) == (R, 2, 9)
    got = ops.score_spatial(gr, ge, gm, 0, table, res["lag"], D)
    cut = ops.score_spatial(gr[..., D:L - D], ge[..., D + lags[0]:L - D + lags[0]], gm[..., D:L - D], 0, table)
    assert torch.equal(got, cut)
    cut = scorer.score(ge[..., D + lags[0]:L - D + lags[0]], gr[..., D:L - D], gm[..., D:L - D], spatial=True)
    assert all(_same(res[k], cut[k]) for k in KEYS)
    want, bound = reference(("align", L), refs, est, mix, [0] * R, [lags[0]] * R, D)
    assert REF.worst(got.cpu().numpy(), want, bound) <= 1.0
    per_ear = torch.stack([ge[:, c, D + lags[c]:L - D + lags[c]] for c in range(2)], dim=1)
    own = scorer.score(per_ear, gr[..., D:L - D], gm[..., D:L - D], spatial=True)
    a, b = res["spatial_whole"][:, 1].cpu().numpy(), own["spatial_whole"][:, 1].cpu().numpy()
    print("ipd_err with both ears at the left ear's lag %s rad; with each ear cut at its own lag %s rad" % (a, b))
    assert (a > 0.1).all() and (b < 0.1 * a).all()


def test_spatial_path_makes_no_host_synchronisation(dev, scorer):
    """torch raises on any synchronising call (a copy from pageable host memory, .item(), a boolean mask) while the mode is "error"."""
    refs, est, mix = batch(3)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    want = scorer.score(ge, gr, gm, target=[0, 1], window=2, spatial=True)
    aligned = scorer.score(ge, gr, gm, target=[0, 1], window=2, align=16, spatial=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = scorer.score(ge, gr, gm, target=[0, 1], window=2, spatial=True)
        res16 = scorer.score(ge, gr, gm, target=[0, 1], window=2, align=16, spatial=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(_same(res[k], want[k]) for k in KEYS) and all(_same(res16[k], aligned[k]) for k in KEYS)


def test_scenario_auralizer_separator_scorer(dev, scorer):
    """Auralizer.render(..., return_images=True) -> estimates -> Scorer(spatial=True): the target image itself has no cue error; its mono
    downmix in both ears has lost exactly the target's level differences; the Separator's binaural output goes through (plumbing)."""
    from m2h.audio.render import Auralizer
    from m2h import synthetic
    from m2h.separate import Separator
    L, Lr = 40000, 96
    rng = np.random.default_rng(3)
    t = np.arange(L) / 16000.0
    src = np.stack([np.stack([0.3 * rng.standard_normal(L) * (1 + 0.5 * np.sin(2 * np.pi * (0.7 + s + r) * t)) for s in range(2)]) for r in range(R)])
    decay = np.exp(-np.arange(Lr) / 20.0)[None, None, :, None]
    rirs = rng.standard_normal((R, 2, Lr, 2)) * decay
    rirs[:, 0, :, 1] *= 0.4                                                              # the target is louder on the left,
    rirs[:, 1, :, 0] *= 0.3                                                              # the interferer on the right
    xs, hs = _gpu(dev, src.astype(np.float32), rirs.astype(np.float32))
    mix, images = Auralizer(dev).render(xs, hs, return_images=True)
    assert tuple(mix.shape) == (R, 2, L) and tuple(images.shape) == (R, 2, 2, L)
    refs = 0.5 * images                                                                 # the sources as they are in the mixture (gains 1 / S)
    same = scorer.score(refs[:, 0], refs, mix, spatial=True)
    for key in ("spatial_whole", "spatial_track"):
        v = same[key]
        assert bool((v[..., :3] == 0).all()) and bool(torch.equal(v[..., 6:], v[..., 3:6])) and bool((v[..., 3:6] > 0).all())
    mono = refs[:, 0].mean(dim=1, keepdim=True).expand(R, 2, L)
    down = scorer.score(mono.contiguous(), refs, mix, spatial=True)
    cues = down["spatial_cues"].cpu().numpy()
    assert (cues[:, :, 1, :, 0] == 0).all() and (cues[:, :, 1, :, 1] == 0).all()         # the same samples in both ears: the same bits in PL and PR, CIM = 0
    hr, hm = refs.cpu().numpy(), mix.cpu().numpy()
    for r in range(R):
        sums, bound = REF.recording_sums(hr[r], hr[r, 0], hm[r])
        ws, wb = REF.window_sums(sums, sums.shape[0], 1)[0], REF.window_sums(bound, sums.shape[0], 1)[0]
        w, ild_g = REF.weights(ws), REF.cues(ws)[0, :, 0]
        want = (w * np.abs(ild_g)).sum() / w.sum()
        tol = REF.ild_bound(ws, wb)[0].max() + 2.0 * np.abs(ild_g).max() * wb[0, :, :2].sum() / (ws[0, :, :2].sum() - wb[0, :, :2].sum())
        got = float(down["spatial_whole"][r, 0])
        print("recording %d: ild_err of the mono downmix %.9f dB, weighted |ILD_G| %.9f dB, tolerance %.3e" % (r, got, want, tol))
        assert want > 1.0 and abs(got - want) <= tol
    sep = Separator(synthetic.make_state_dict(synthetic.policy_shapes(), 2), dev, math=ops.MATH_FP32)
    y = sep.separate(mix, [4, 7], output="binaural")
    assert tuple(y.shape) == (R, 2, L)
    out = scorer.score(y, refs, mix, spatial=True)
    M = out["plan"]["M"]
    assert tuple(out["spatial_whole"].shape) == (R, 9) and tuple(out["spatial_track"].shape) == (R, M, 9) and tuple(out["spatial_cues"].shape) == (R, M, 3, 32, 3)
    assert bool(torch.isfinite(out["spatial_whole"]).all()) and bool(torch.isfinite(out["spatial_track"]).all())


def test_cli_spatial_rows_and_json(dev, tmp_path):
    """score.py --spatial --json on small float32 two-channel WAVs: the new keys match the float64 definition within the bound that follows
    from the sums' and the printed rows are the JSON's; without the flag none of the new keys and none of the rows appear; mono files are
    refused."""
    S, L = 2, 20001
    refs, est, mix = (a[0, ..., :L] for a in batch(3))
    refs = refs[:S]
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1", "mono")}
    for k, v in (("est", est), ("mix", mix), ("ref0", refs[0]), ("ref1", refs[1])):
        _write_wav(p[k], np.ascontiguousarray(v.T))
    _write_wav(p["mono"], np.ascontiguousarray(est[0]))
    out_json = str(tmp_path / "scores.json")
    cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"], "--reference", p["ref1"],
           "--json", out_json]
    run = lambda c: subprocess.run(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)   # noqa: E731
    res = run(cmd + ["--spatial"])
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    sums, bound = REF.recording_sums(refs, est, mix, 0)                                 # [J, 3, 32, 4]
    J = sums.shape[0]
    assert got["spatial_metrics"] == list(REF.ORDER) and np.array(got["spatial_track"]).shape == (J, 9)
    assert np.array(got["spatial_cues"]).shape == (J, 3, 32, 3)
    for values, s, b in ((got["spatial_whole"], REF.window_sums(sums, J, 1)[0], REF.window_sums(bound, J, 1)[0]), (got["spatial_track"], sums, bound)):
        want, tol = REF.metrics(s), REF.metrics_bound(s, b)
        assert np.isfinite(tol).all() and (np.abs(np.asarray(values) - want) <= tol).all(), (values, want, tol)
    d = np.abs(np.asarray(got["spatial_cues"]) - REF.cues(sums))
    assert (d <= REF.cues_bound(sums, bound)).all()
    assert np.allclose(got["spatial_track_mean"], np.mean(got["spatial_track"], axis=0), rtol=1e-12, atol=0)
    assert np.allclose(got["spatial_track_median"], np.median(got["spatial_track"], axis=0), rtol=1e-12, atol=0)
    lines = res.stdout.splitlines()
    for label, key in (("spatial whole", "spatial_whole"), ("spatial window mean", "spatial_track_mean"), ("spatial window median", "spatial_track_median")):
        row = [ln for ln in lines if ln.startswith("%-8s %-23s" % ("binaural", label))]
        assert len(row) == 1, res.stdout
        assert np.allclose([float(v) for v in row[0][32:].split()], got[key], rtol=1e-11, atol=0), (label, row[0])
    for name in ("left", "right"):                                                      # the existing rows: still one of each
        for label in ("whole", "window mean", "window median"):
            assert len([ln for ln in lines if ln.startswith("%-8s %-14s" % (name, label))]) == 1, res.stdout
    with_flag = got
    res = run(cmd)
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    assert not [k for k in got if k.startswith("spatial")]
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith(("spatial", "binaural")) or "spatial w" in ln]
    assert json.dumps({k: v for k, v in with_flag.items() if not k.startswith("spatial")}) == json.dumps(got)
    mono_cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["mono"], "--mixture", p["mix"], "--reference", p["mono"], "--spatial"]
    res = run(mono_cmd)
    assert res.returncode != 0 and "two channels are needed" in res.stdout, res.stdout
