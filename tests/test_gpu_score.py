"""GPU: m2h.audio.score (the Scorer, csrc/score.hip) against its float64 definition (tests/score_ref.py).

Bounds.  The tile Grams against np.longdouble sums, every entry: |got - want| <= (ceil(tile / 256) + 16) 2^-52 sum|a b| -- products are
exact, so only the additions round: a thread's chain of at most ceil(tile / 256) of them, then the block's tree of 6 + 3.  The scores
against score_direct_f64: 1e-6 dB, about 2 500 times the float64 algebra's worst error on the CPU (tests/test_score_cpu.py), 13 times
below the best an fp32 Gram reaches there and far below every defect that file lists.  The batch, the window's position, the strides and
the alignment of a row do not change the arithmetic or its order: those comparisons are bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_ref as REF
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 2
TILE = 16000


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scorer(dev):
    from m2h.audio.score import Scorer
    return Scorer(dev)


_inputs = {}


def batch(S, L, seed, C=1, snr43=False):
    """R recordings of score_ref.inputs: refs [R, S, C, L], est [R, C, L], mix [R, 2, L]; made once, shared and read-only"""
    key = (S, L, seed, C, snr43)
    if key not in _inputs:
        _inputs[key] = tuple(np.stack(a) for a in zip(*[REF.inputs(S, L, seed + 50 * r, C, snr43) for r in range(R)]))
        for a in _inputs[key]:
            a.setflags(write=False)
    return _inputs[key]


def _gpu(dev, *arrays):
    return [torch.tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]      # (a copy: the shared inputs are read-only)


def _score_args(refs, est, mix, C):
    """the public shapes: [R, S, L] and [R, L] for C = 1"""
    return (est[:, 0], refs[:, :, 0], mix) if C == 1 else (est, refs, mix)


def _same(a, b):
    """bit for bit, NaN in the same places"""
    return a.shape == b.shape and bool(torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))) and \
        bool(torch.equal(torch.isnan(a), torch.isnan(b)))


@pytest.mark.parametrize("L,tile", [(1, TILE), (15999, TILE), (16001, TILE), (40001, TILE), (40, 7)])
def test_tile_grams_against_long_double(dev, L, tile):
    refs, est, mix = batch(6, 40001, 21, C=2)
    refs, est, mix = refs[..., :L], est[..., :L], mix[..., :L]
    J = -(-L // tile)
    want = np.zeros((R, 2, J, 54), np.longdouble)
    scale = np.zeros((R, 2, J, 54))
    for r in range(R):
        for c in range(2):
            for j in range(J):
                t0, t1 = j * tile, min((j + 1) * tile, L)
                want[r, c, j] = REF.gram_f64(REF.gram_rows(refs[r], est[r], mix[r], c, t0, t1, np.longdouble), np.longdouble)
                scale[r, c, j] = REF.gram_abs(REF.gram_rows(refs[r], est[r], mix[r], c, t0, t1))
    bound = (-(-tile // 256) + 16) * 2.0 ** -52 * scale
    gr, ge, gm = _gpu(dev, refs, est, mix)
    worst = 0.0
    for C in (1, 2):
        for S in (1, 3, 6):
            N = S + 3
            sig = list(range(S)) + [6, 7, 8]                                     # these signals among the nine of S = 6
            pos = {(i, k): 9 + i * 9 - i * (i - 1) // 2 + k - i for i in range(9) for k in range(i, 9)}
            cols = sig + [pos[(sig[i], sig[k])] for i in range(N) for k in range(i, N)]
            got = ops.score_gram(gr[:, :S, :C], ge[:, :C], gm, tile)             # views of the S = 6, C = 2 tensors, read in place
            assert ops.last_kernel() == "score_gram" and got.dtype == torch.float64 and tuple(got.shape) == (R, C, J, len(cols))
            got = got.cpu().numpy()
            err = np.abs(got.astype(np.longdouble) - want[:, :C][..., cols]).astype(np.float64)
            assert np.isfinite(got).all() and (err <= bound[:, :C][..., cols]).all(), (C, S, float((err / bound[:, :C][..., cols]).max()))
            worst = max(worst, float((err / np.maximum(scale[:, :C][..., cols], 1e-300)).max() * 2.0 ** 52))
    print("tile Grams L=%d tile=%d: largest error %.2f x 2^-52 sum|ab| of a bound of %d" % (L, tile, worst, -(-tile // 256) + 16))


CASES = [(1, 16000, False), (2, 15999, False), (3, 40001, False), (3, 5, False), (6, 40001, False), (3, 40001, True)]   # tests/test_score_cpu.py


@pytest.mark.parametrize("S,L,snr43", CASES)
def test_scores_match_the_direct_float64_definition(dev, scorer, S, L, snr43):
    cols = REF.WELL if S == 1 else REF.ALL
    worst = 0.0
    for C in (1, 2):
        refs, est, mix = batch(S, L, 7 + S, C, snr43)
        gr, ge, gm = _gpu(dev, refs, est, mix)
        for window, hop in ((1, 1), (2, 1)):
            res = scorer.score(*_score_args(gr, ge, gm, C), window=window, hop=hop)
            assert ops.last_kernel() == "score_windows"
            M = res["plan"]["M"]
            assert res["whole"].dtype == torch.float64 and tuple(res["whole"].shape) == (R, C, 11) and tuple(res["track"].shape) == (R, C, M, 11)
            assert res["active"].dtype == torch.bool and tuple(res["active"].shape) == (R, C, M) and bool(res["active"].all())
            whole, track = res["whole"].cpu().numpy(), res["track"].cpu().numpy()
            for r in range(R):
                want_whole, want_track = REF.score_direct_f64(refs[r], est[r], mix[r], 0, TILE, window, hop)
                assert np.isfinite(want_track[..., list(cols)]).all()
                e = max(REF.max_err(whole[r], want_whole, cols), REF.max_err(track[r], want_track, cols))
                worst = max(worst, e)
                assert e <= REF.TOL_GPU, (C, window, hop, r, e)
    print("scores S=%d L=%d snr43=%s: largest error %.3e dB of %.0e" % (S, L, snr43, worst, REF.TOL_GPU))


def test_targets_per_recording(dev, scorer):
    refs, est, mix = batch(3, 40001, 10, 2)
    est = np.stack([est[0], (0.7 * refs[1, 1] + 0.1 * est[1]).astype(np.float32)])        # recording 1 estimates source 1
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=[0, 1])
    for r, t in enumerate((0, 1)):
        want_whole, want_track = REF.score_direct_f64(refs[r], est[r], mix[r], t, TILE)
        assert max(REF.max_err(res["whole"][r].cpu().numpy(), want_whole), REF.max_err(res["track"][r].cpu().numpy(), want_track)) <= REF.TOL_GPU
        solo = scorer.score(ge[r:r + 1], gr[r:r + 1], gm[r:r + 1], target=t)
        assert _same(solo["whole"][0], res["whole"][r]) and _same(solo["track"][0], res["track"][r])


def test_batch_slices_strides_and_alignment_are_bit_identical(dev, scorer):
    S, L, C = 3, 40001, 2
    refs, est, mix = batch(S, L, 10, C)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, window=2, hop=1)
    one = scorer.score(ge, gr, gm)
    # each recording of the batch against its solo score
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), window=2, hop=1)
        assert _same(solo["whole"][0], res["whole"][r]) and _same(solo["track"][0], res["track"][r]) and bool(torch.equal(solo["active"][0], res["active"][r]))
    # track[m] against the whole of that slice scored alone (slice starts at tile multiples)
    for plan_res in (res, one):
        for m, (t0, t1) in enumerate(plan_res["plan"]["samples"]):
            alone = scorer.score(ge[..., t0:t1], gr[..., t0:t1], gm[..., t0:t1])
            assert _same(alone["whole"], plan_res["track"][:, :, m]), (m, t0, t1)
    # strided views against contiguous copies: references sliced out of a larger `images`, an estimate viewed from a larger buffer
    images = torch.zeros((R + 1, S + 2, C, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    strided = scorer.score(*views, window=2, hop=1)
    assert _same(strided["whole"], res["whole"]) and _same(strided["track"], res["track"])
    # odd L misaligns every second row of the contiguous tensors; the same data in buffers whose rows are all 16-byte aligned
    assert L % 4 == 1 and all(t.data_ptr() % 16 == 0 for t in (gr, ge, gm))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (3,), device=dev)], dim=-1)[..., :L]   # noqa: E731  (row stride L + 3 = 40004)
    aligned = scorer.score(pad(ge), pad(gr), pad(gm), window=2, hop=1)
    assert _same(aligned["whole"], res["whole"]) and _same(aligned["track"], res["track"])
    # the mono form of the same call: channel 0 of the two-channel tile Grams
    g2, g1 = ops.score_gram(gr, ge, gm, TILE), ops.score_gram(gr[:, :, :1], ge[:, :1], gm, TILE)
    assert torch.equal(g1, g2[:, :1])


def test_rows_past_two_to_the_31_elements(dev, scorer):
    """An estimate whose second row starts 2^31 + 8 elements after the first (a view of a larger buffer): the strides are 64-bit."""
    S, L = 1, 16001
    refs, est, mix = batch(S, L, 4)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    stride = 2 ** 31 + 8
    buf = torch.empty((stride + L + 8,), device=dev)
    view = buf.as_strided((R, 1, L), (stride, L, 1), 3)
    view.copy_(ge)
    assert view.stride(0) > 2 ** 31 and view.data_ptr() % 16 != 0
    far, near = scorer.score(view, gr, gm), scorer.score(ge, gr, gm)
    assert _same(far["whole"], near["whole"]) and _same(far["track"], near["track"])
    assert REF.max_err(near["whole"][1].cpu().numpy(), REF.score_direct_f64(refs[1], est[1], mix[1])[0], REF.WELL) <= REF.TOL_GPU


def test_per_second_track_against_bss_metrics(dev, scorer):
    """S = 1: the per-second track agrees with m2h_bss_metrics on the same seconds within that kernel's own 2e-3 dB."""
    refs, est, mix = batch(1, 48000, 13)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    track = scorer.score(ge[:, 0], gr[:, :, 0], gm)["track"][:, 0].cpu().numpy()                          # [R, 3, 11]
    sec = lambda t: t.reshape(-1, 16000).contiguous()                                                   # noqa: E731
    old = ops.bss_metrics(sec(gr[:, 0, 0]), sec(ge[:, 0]), sec(gm[:, 0]), sec(gm[:, 1])).cpu().numpy().reshape(R, 3, 11)
    d = np.abs(track - old)[..., list(REF.WELL)].max()
    print("per-second track vs m2h_bss_metrics: %.3e dB" % d)
    assert d <= 2e-3


def test_degenerate_windows_on_the_gpu(dev, scorer):
    """A silent second (target and all), a silent interferer, h > w with an empty last window, L = 1."""
    refs, est, mix = (np.array(a) for a in batch(3, 40001, 10))
    refs[0, :, :, 16000:32000] = 0.0                                               # recording 0: every source silent in second 1
    refs[1, 1] = 0.0                                                               # recording 1: a silent interferer throughout
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge[:, 0], gr[:, :, 0], gm)
    assert res["active"][:, 0].cpu().tolist() == [[True, False, True], [True, True, True]]
    assert bool(torch.isnan(res["track"][0, 0, 1]).all()) and bool(torch.isfinite(res["track"][1]).all()) and bool(torch.isfinite(res["whole"]).all())
    for r in range(R):
        want_whole, want_track = REF.score_direct_f64(refs[r], est[r], mix[r])
        assert max(REF.max_err(res["whole"][r].cpu().numpy(), want_whole), REF.max_err(res["track"][r].cpu().numpy(), want_track)) <= REF.TOL_GPU
    res = scorer.score(ge[:, 0, :70], gr[:, :, 0, :70], gm[..., :70], tile=7, window=2, hop=5)
    assert res["plan"]["samples"] == [(0, 14), (35, 49), (70, 70)] and res["active"][1, 0].cpu().tolist() == [True, True, False]
    assert bool(torch.isnan(res["track"][:, :, 2]).all()) and bool(torch.isfinite(res["track"][1, :, :2]).all())
    res = scorer.score(ge[:, 0, :1], gr[:, :, 0, :1], gm[..., :1])
    assert bool(torch.isnan(res["whole"]).all()) and not bool(res["active"].any())


def test_score_makes_no_host_synchronisation(dev, scorer):
    """torch raises on any synchronising call (a copy from pageable host memory, .item(), a boolean mask) while the mode is "error"."""
    refs, est, mix = batch(3, 40001, 10, 2)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    want = scorer.score(ge, gr, gm, target=[0, 1], window=2)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = scorer.score(ge, gr, gm, target=[0, 1], window=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same(res["track"], want["track"]) and _same(res["whole"], want["whole"])


def test_argument_errors_launch_nothing(dev, scorer):
    from test_score_cpu import scorer_argument_errors
    lib = _lib.load()
    ok, bad = scorer_argument_errors(dev)
    scorer.score(**ok)
    n0 = lib.m2h_launch_count()
    for exc, pattern, kw in bad:
        with pytest.raises(exc, match=pattern):
            scorer.score(**dict(ok, **kw))
    with pytest.raises(ValueError, match="mixture must live on cuda:0, got cpu"):
        scorer.score(**dict(ok, mixture=ok["mixture"].cpu()))
    with pytest.raises(TypeError, match="host integers"):
        scorer.score(**dict(ok, target=torch.zeros((2,), dtype=torch.int64, device=dev)))
    assert lib.m2h_launch_count() == n0


def _write_wav(path, rate, data):
    from scipy.io import wavfile
    wavfile.write(path, rate, data)


def test_cli_render_images_then_score(dev, tmp_path):
    """render.py --out-image writes every source's image as --out-target writes the first; score.py on those files and an estimate prints
    and writes what score_direct_f64 gives on the same WAV samples; a 44.1 kHz file and a mono / stereo mismatch are refused."""
    from scipy.io import wavfile
    import render_ref as RREF
    r = np.random.default_rng(5)
    La, Lb = 36001, 36001          # (equal lengths: an interferer that falls silent leaves one source in the projection, whose SI-SIR is rounding noise)
    a = np.clip(np.round(3000 * r.standard_normal(La)), -32768, 32767).astype(np.int16)
    b = np.clip(np.round(3000 * r.standard_normal(Lb)), -32768, 32767).astype(np.int16)
    ha = np.round(32768 * 0.05 * RREF.make_rirs(1, 1, 1, 3000, 8)[0, 0, 0]).astype(np.int16)
    hb = np.round(32768 * 0.05 * RREF.make_rirs(1, 1, 1, 2000, 9)[0, 0, 0]).astype(np.int16)
    p = {k: str(tmp_path / (k + ".wav")) for k in ("a", "b", "ha", "hb", "mix", "target", "img0", "img1", "est", "est1", "a44")}
    for k, v in (("a", a), ("b", b), ("ha", ha), ("hb", hb)):
        _write_wav(p[k], 16000, v)
    run = lambda *cmd: subprocess.run([sys.executable] + list(cmd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)   # noqa: E731
    res = run(os.path.join(ROOT, "render.py"), "--source", p["a"], "--rir", p["ha"], "--source", p["b"], "--rir", p["hb"], "--gain", "0.6", "--gain", "0.3",
              "--out", p["mix"], "--out-target", p["target"], "--out-image", p["img0"], "--out-image", p["img1"])
    assert res.returncode == 0, res.stdout
    wavs = {k: wavfile.read(p[k])[1] for k in ("mix", "target", "img0", "img1")}
    assert all(w.dtype == np.int16 and w.shape == (La, 2) for w in wavs.values())
    assert np.array_equal(wavs["img0"], wavs["target"]) and np.abs(wavs["img1"]).max() > 100 and not np.array_equal(wavs["img1"], wavs["img0"])
    assert np.abs(wavs["mix"].astype(np.int64) - wavs["img0"] - wavs["img1"]).max() <= 2       # the images at their gains add up to the mixture
    res = run(os.path.join(ROOT, "render.py"), "--source", p["a"], "--rir", p["ha"], "--out", p["mix"] + "x", "--out-image", p["img0"] + "x", "--out-image", p["img1"] + "x")
    assert res.returncode != 0 and "2 --out-image for 1 sources" in res.stdout
    # a binaural estimate: most of the target, some of the interferer, noise
    est = np.clip(np.rint(0.8 * wavs["img0"] + 0.1 * wavs["img1"] + 20 * r.standard_normal((La, 2))), -32768, 32767).astype(np.int16)
    _write_wav(p["est"], 16000, est)
    out_json = str(tmp_path / "scores.json")
    res = run(os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["img0"], "--reference", p["img1"], "--json", out_json)
    assert res.returncode == 0, res.stdout
    f = lambda w: (w.astype(np.float32) * np.float32(1.0 / 32768.0)).T                                  # noqa: E731
    want_whole, want_track = REF.score_direct_f64(np.stack([f(wavs["img0"]), f(wavs["img1"])]), f(est), f(wavs["mix"]))
    got = json.load(open(out_json))
    assert got["metrics"] == list(REF.O.BSS_METRIC_ORDER) and got["channels"] == ["left", "right"] and got["windows"][-1] == [32000, La]
    print("score.py JSON: whole %.3e dB, track %.3e dB of %.0e" % (REF.max_err(got["whole"], want_whole), REF.max_err(got["track"], want_track), REF.TOL_GPU))
    assert REF.max_err(got["whole"], want_whole) <= REF.TOL_GPU and REF.max_err(got["track"], want_track) <= REF.TOL_GPU
    assert got["active"] == [[True] * 3] * 2 and REF.max_err(got["track_mean"], want_track.mean(axis=1)) <= REF.TOL_GPU
    assert REF.max_err(got["track_median"], np.median(want_track, axis=1)) <= REF.TOL_GPU
    lines = res.stdout.splitlines()
    for c, name in enumerate(("left", "right")):
        for label, want in (("whole", want_whole[c]), ("window mean", want_track[c].mean(axis=0)), ("window median", np.median(want_track[c], axis=0))):
            row = [ln for ln in lines if ln.startswith("%-8s %-14s" % (name, label))]
            assert len(row) == 1, res.stdout
            assert REF.max_err([float(v) for v in row[0][23:].split()], want) <= REF.TOL_GPU, (name, label, row[0])
    # refused: another sample rate (both rates named), a mono estimate against two-channel references (both counts named), unequal lengths
    _write_wav(p["a44"], 44100, est)
    res = run(os.path.join(ROOT, "score.py"), "--estimate", p["a44"], "--mixture", p["mix"], "--reference", p["img0"])
    assert res.returncode != 0 and "44100 Hz" in res.stdout and "16000 Hz is required" in res.stdout
    _write_wav(p["est1"], 16000, est[:, 0])
    res = run(os.path.join(ROOT, "score.py"), "--estimate", p["est1"], "--mixture", p["mix"], "--reference", p["img0"])
    assert res.returncode != 0 and "has 1 channel and" in res.stdout and "has 2" in res.stdout
    _write_wav(p["est1"], 16000, est[:-1])
    res = run(os.path.join(ROOT, "score.py"), "--estimate", p["est1"], "--mixture", p["mix"], "--reference", p["img0"])
    assert res.returncode != 0 and "%d samples long" % (La - 1) in res.stdout and "is %d" % La in res.stdout


def test_render_separate_score_plumbing(dev, scorer):
    """Plumbing only: a rendered 2.5 s mixture with its images through Separator.separate(output="binaural") with synthetic weights into
    Scorer.score; shapes, and finite numbers wherever a window is active.  No quality claim."""
    import render_ref as RREF
    from m2h import synthetic
    from m2h.audio.render import Auralizer
    from m2h.separate import Separator
    x, h = _gpu(dev, RREF.make_sources(2, 2, 40000, 11), 0.05 * RREF.make_rirs(2, 2, 1, 8000, 11)[:, :, 0])
    mix, images = Auralizer(dev).render(x, h, return_images=True)
    sep = Separator(synthetic.make_state_dict(synthetic.policy_shapes(), 2), dev, math=ops.MATH_FP32)
    y = sep.separate(mix, 4, use_memory=False, output="binaural")
    assert tuple(y.shape) == (2, 2, 40000)
    res = scorer.score(y, images * 0.5, mix)
    assert tuple(res["whole"].shape) == (2, 2, 11) and tuple(res["track"].shape) == (2, 2, 3, 11) and tuple(res["active"].shape) == (2, 2, 3)
    assert bool(res["active"].all()) and bool(torch.isfinite(res["track"][res["active"]]).all()) and bool(torch.isfinite(res["whole"]).all())
    mono = scorer.score(sep.separate(mix, 4, use_memory=False), images[:, :, 0], mix)                    # a mono estimate against the left images
    assert tuple(mono["whole"].shape) == (2, 1, 11) and bool(torch.isfinite(mono["track"][mono["active"]]).all())


CLI_JSON_KEYS = ["estimate", "mixture", "references", "sample_rate", "samples", "channels", "window_s", "hop_s",
                 "metrics", "whole", "track_mean", "track_median", "active_windows", "windows", "track", "active",
                 "spectral_metrics", "spectral_whole", "spectral_track", "spectral_track_mean", "spectral_track_median",
                 "spatial_metrics", "spatial_whole", "spatial_track", "spatial_track_mean", "spatial_track_median", "spatial_cues",
                 "itd_metrics", "itd_whole", "itd_track", "itd_track_mean", "itd_track_median", "itd_gcc",
                 "stoi_metrics", "stoi_whole", "stoi_track", "stoi_track_mean", "stoi_track_median", "stoi_frames",
                 "bss_taps", "bss_metrics", "bss_whole", "bss_track", "bss_track_mean", "bss_track_median",
                 "align", "region", "lag", "lag_track"]


def test_cli_every_family_at_once_is_the_summary_of_the_same_call(dev, tmp_path):
    """score.py with every flag at once on int16 two-channel WAVs (the planted pair of tests/itd_ref.py, S = 2, L = 40001): every family
    block of the JSON is summarize(Scorer.score(...)) of the same samples scored in this process, number for number (the kernels'
    bits do not depend on the process); the JSON's keys come in their fixed order; the table's header and each family's appear once,
    in the order table, spectral, spatial, itd, stoi, bss."""
    import itd_ref
    from m2h.audio.score import Scorer, summarize
    S, L = 2, 40001
    refs, est, mix = itd_ref.planted(0, L, S)
    q = lambda a: np.clip(np.rint(np.asarray(a, np.float64) * 32768.0), -32768, 32767).astype(np.int16)      # noqa: E731
    back = lambda a: a.astype(np.float32) * np.float32(1.0 / 32768.0)                                        # noqa: E731
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1")}
    for k, v in (("est", est), ("mix", mix), ("ref0", refs[0]), ("ref1", refs[1])):
        _write_wav(p[k], 16000, np.ascontiguousarray(q(v).T))
    out_json = str(tmp_path / "scores.json")
    cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"], "--reference", p["ref1"],
           "--align", "16", "--window", "2", "--hop", "1", "--spectral", "--spatial", "--itd", "--stoi", "--bss", "8", "--json", out_json]
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)       # (stdout alone: libraries may write to stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    got = json.load(open(out_json))
    assert list(got) == CLI_JSON_KEYS
    ge, gr, gm = _gpu(dev, back(q(est))[None], back(q(refs))[None], back(q(mix))[None])
    res = Scorer(dev).score(ge, gr, gm, target=0, window=2, hop=1, align=16, spectral=True, spatial=True, stoi=True, bss=8, itd=True)
    s = summarize(res)
    assert res["plan"]["M"] == 2 and got["windows"] == [list(w) for w in res["plan"]["samples"]] and got["bss_taps"] == 8
    for prefix in ("", "spectral_", "spatial_", "itd_", "stoi_", "bss_"):
        want = {prefix + "metrics": s[prefix + "metrics"], prefix + "track": res[prefix + "track"][0].tolist()}
        want.update({prefix + k: s[prefix + k][0] for k in ("whole", "track_mean", "track_median")})
        for key, value in want.items():
            assert json.dumps(got[key]) == json.dumps(value), key
    for key in ("spatial_cues", "itd_gcc", "stoi_frames", "active", "lag", "lag_track"):
        assert json.dumps(got[key]) == json.dumps(res[key][0].tolist()), key
    assert json.dumps(got["active_windows"]) == json.dumps(s["active_windows"][0])
    heads = [ln[:8].rstrip() for ln in run.stdout.splitlines() if not ln.startswith(("left", "right", "binaural", "score.py:"))]
    assert heads == ["channel", "spectral", "spatial", "itd us", "stoi", "bss 8"], run.stdout
