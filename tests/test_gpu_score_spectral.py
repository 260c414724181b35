"""The Scorer's STFT distance on the GPU (m2h/audio/score.py "Spectral", csrc/score_spectral.hip): the seven tile sums against the float64
definition of tests/spectral_ref.py within its bound, Scorer.score(..., spectral=True) and its bit-identical properties, alignment, the
one-second relation to eval_metrics.STFT_L2_distance, no host synchronisation, argument errors and the command line.

Measured on an MI355X (worst error / bound over the cases of test_tile_sums_against_the_float64_definition): see DESIGN.md §8.8."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spectral_ref as REF
from score_cases import LMAX, R, _gpu, _same, _target, _write_wav, batch, recordings, targets
from m2h import _lib, ops
from m2h.audio import score as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return recordings("clicks", lambda r: REF.clicks(seed=r))


def reference(key, refs, est, mix, tg, lag=None, D=0):
    """(sums [R, C, J, 7], bound [R, C, J, 7]) float64 of a batch; computed once per key"""
    return recordings(("spectral", key), lambda r: REF.recording_sums(refs[r], est[r], mix[r], tg[r], None if lag is None else lag[r], D))


@pytest.mark.parametrize("C,S,L", [(C, S, L) for C, S in ((1, 1), (1, 3), (2, 1), (2, 3)) for L in (1, 5, 700, 15999, 16000, 16001, 40001)]
                         + [(1, 1, "clicks")])
def test_tile_sums_against_the_float64_definition(dev, table, C, S, L):
    """L = 1 and 16001 are the smallest shapes at which zero extension, reflection and the second tile can go wrong; the clicks show frame
    placement, which noise-like inputs hide."""
    if L == "clicks":
        refs, est, mix = click_batch()
    else:
        refs, est, mix = (a[..., :L] for a in batch(S, C))
    tg = targets(S)
    want, bound = reference((C, S, L), refs, est, mix, tg)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    got = ops.score_spectral(gr, ge, gm, _target(dev, tg), table)
    torch.cuda.synchronize()
    assert ops.last_kernel() == "score_spectral" and got.dtype == torch.float64 and tuple(got.shape) == want.shape
    w = REF.worst(got.cpu().numpy(), want, bound)
    print("score_spectral C = %d, S = %d, L = %s: worst error / bound %.3e" % (C, S, L, w))
    assert w <= 1.0


@pytest.mark.parametrize("window,hop", [(1, 1), (2, 1)])
def test_scorer_spectral_is_spectral_from_sums_of_the_windowed_sums(dev, scorer, table, window, hop):
    C, S = 2, 3
    refs, est, mix = batch(S, C)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, window=window, hop=hop, spectral=True)
    plain = scorer.score(ge, gr, gm, target=tg, window=window, hop=hop)
    J, M = res["plan"]["J"], res["plan"]["M"]
    assert "spectral_whole" not in plain and "spectral_track" not in plain
    assert res["spectral_whole"].dtype == torch.float64 and tuple(res["spectral_whole"].shape) == (R, C, 8)
    assert res["spectral_track"].dtype == torch.float64 and tuple(res["spectral_track"].shape) == (R, C, M, 8)
    for k in ("whole", "track"):                                                        # the eleven BSS numbers do not move by a bit
        assert _same(res[k], plain[k])
    assert bool(torch.equal(res["active"], plain["active"]))
    tiles = ops.score_spectral(gr, ge, gm, _target(dev, tg), table)
    q = torch.tensor([j1 - j0 for j0, j1 in res["plan"]["tiles"]], dtype=torch.float64).to(dev)
    assert _same(res["spectral_whole"], SC.spectral_from_sums(ops.score_windows(tiles, 1, J, 1), float(J))[:, :, 0])
    assert _same(res["spectral_track"], SC.spectral_from_sums(ops.score_windows(tiles, M, window, hop), q))
    # and the numbers themselves against the definition, within the bound that follows from the sums'
    want, bound = reference((C, S, LMAX), refs, est, mix, tg)
    wsum, Q = REF.window_sums(want, window, hop)
    wbound, _ = REF.window_sums(bound, window, hop)
    d = np.abs(res["spectral_track"].cpu().numpy()[..., [0, 1, 3, 4]] - REF.metrics(wsum, Q)[..., [0, 1, 3, 4]])
    assert (d <= REF.metrics_bound(wsum, wbound, Q)).all()


def test_batch_slices_strides_and_alignment_are_bit_identical(dev, scorer):
    S, L, C = 3, LMAX, 2
    refs, est, mix = batch(S, C)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    keys = ("spectral_whole", "spectral_track")
    res = scorer.score(ge, gr, gm, window=2, hop=1, spectral=True)
    one = scorer.score(ge, gr, gm, spectral=True)
    # each recording of the batch against its solo score
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), window=2, hop=1, spectral=True)
        assert all(_same(solo[k][0], res[k][r]) for k in keys)
    # track[m] against that slice scored as a whole (slices start at tile multiples)
    for plan_res in (res, one):
        for m, (t0, t1) in enumerate(plan_res["plan"]["samples"]):
            alone = scorer.score(ge[..., t0:t1], gr[..., t0:t1], gm[..., t0:t1], spectral=True)
            assert _same(alone["spectral_whole"], plan_res["spectral_track"][:, :, m]), (m, t0, t1)
    # strided views inside larger buffers against contiguous copies
    images = torch.zeros((R + 1, S + 2, C, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    strided = scorer.score(*views, window=2, hop=1, spectral=True)
    assert all(_same(strided[k], res[k]) for k in keys)
    # odd L puts every second row of the contiguous tensors at an odd element offset; the same data in rows that are all 16-byte aligned
    assert L % 4 == 1 and all(t.data_ptr() % 16 == 0 for t in (gr, ge, gm))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (3,), device=dev)], dim=-1)[..., :L]   # noqa: E731  (row stride L + 3 = 40004)
    aligned = scorer.score(pad(ge), pad(gr), pad(gm), window=2, hop=1, spectral=True)
    assert all(_same(aligned[k], res[k]) for k in keys)
    # the mono form reads channel 0's target and estimate: sums 0, 1, 3, 4 of the two-channel call's left ear
    t2, t1 = ops.score_spectral(gr, ge, gm, 0, scorer._spectral_table()), ops.score_spectral(gr[:, :, :1], ge[:, :1], gm, 0, scorer._spectral_table())
    assert torch.equal(t1[..., [0, 1, 3, 4]], t2[:, :1][..., [0, 1, 3, 4]])


def test_alignment_reads_the_estimate_at_the_lag(dev, scorer):
    """align=64 on an estimate that is the target delayed by 37 samples plus noise: the lag found is 37, and the spectral numbers are, bit
    for bit, those of slices cut by hand at that lag and passed without align."""
    D, lag, S, C = 64, 37, 3, 2
    L = 2 * D + 16001
    refs, _, mix = (a[..., :L] for a in batch(S, C))
    tg = targets(S)
    rng = np.random.default_rng(9)
    est = np.zeros((R, C, L), np.float32)
    for r in range(R):
        est[r, :, lag:] = refs[r, tg[r], :, :L - lag]
    est += (0.01 * rng.standard_normal(est.shape)).astype(np.float32)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, align=D, spectral=True)
    assert res["lag"].cpu().tolist() == [[lag] * C] * R
    cut = scorer.score(ge[..., D + lag:L - D + lag], gr[..., D:L - D], gm[..., D:L - D], target=tg, spectral=True)
    assert _same(res["spectral_whole"], cut["spectral_whole"]) and _same(res["spectral_track"], cut["spectral_track"])
    assert res["plan"]["J"] == 2 and tuple(res["spectral_track"].shape) == (R, C, 2, 8)
    want, bound = reference(("align", L), refs, est, mix, tg, [[lag] * C] * R, D)
    got = ops.score_spectral(gr, ge, gm, _target(dev, tg), scorer._spectral_table(), res["lag"], D)
    assert REF.worst(got.cpu().numpy(), want, bound) <= 1.0


def test_one_second_against_stft_l2_distance(dev, scorer):
    """stft_l2 of one-second recordings against eval_metrics.STFT_L2_distance(...)[1] fed from the STFT feeder's magnitudes and phases;
    tolerance: the bound plus 32768 * 2^-24 relative, the worst case of that kernel's own fp32 mean over 2 F T = 32768 terms."""
    from m2h.audio.stft import STFT
    from m2h.common import eval_metrics
    refs, est, mix = (a[..., :REF.TILE] for a in batch(1, 1))
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge[:, 0], gr[:, :, 0], gm, spectral=True)
    stft = STFT(dev)
    gmag, gph = stft(gr[:, 0], mode=0, want_phase=True)                                 # [R, 512, 32, 1]
    emag, _ = stft(ge, mode=0, want_phase=True)
    gt = torch.cat([gmag, gph], dim=-1)
    zeros = torch.zeros((R, REF.F, REF.T, 2), device=dev)
    dm = eval_metrics.STFT_L2_distance(zeros, zeros, torch.cat([gt, gt], dim=-1), emag, gt)[1]
    got = res["spectral_whole"][:, 0, 0].cpu().numpy()
    want, bound = reference((1, 1, REF.TILE), refs, est, mix, [0] * R)
    for r in range(R):
        tol = REF.metrics_bound(want[r, 0, 0], bound[r, 0, 0], 1.0)[0] + 32768 * 2.0 ** -24 * got[r]
        print("recording %d: STFT_L2_distance %.9e, stft_l2 %.9e, tolerance %.3e" % (r, float(dm[r, 0]), got[r], tol))
        assert abs(float(dm[r, 0]) - got[r]) <= tol
        assert REF.worst(res["spectral_track"][r, 0, 0, 0].item(), REF.metrics(want[r, 0, 0], 1.0)[0], REF.metrics_bound(want[r, 0, 0], bound[r, 0, 0], 1.0)[0]) <= 1.0


def test_spectral_path_makes_no_host_synchronisation(dev, scorer):
    """torch raises on any synchronising call (a copy from pageable host memory, .item(), a boolean mask) while the mode is "error"."""
    refs, est, mix = batch(3, 2)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    want = scorer.score(ge, gr, gm, target=[0, 1], window=2, spectral=True)
    aligned = scorer.score(ge, gr, gm, target=[0, 1], window=2, align=16, spectral=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = scorer.score(ge, gr, gm, target=[0, 1], window=2, spectral=True)
        res16 = scorer.score(ge, gr, gm, target=[0, 1], window=2, align=16, spectral=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same(res["spectral_track"], want["spectral_track"]) and _same(res["spectral_whole"], want["spectral_whole"])
    assert _same(res16["spectral_track"], aligned["spectral_track"]) and _same(res16["spectral_whole"], aligned["spectral_whole"])


def test_argument_errors_launch_nothing(dev, scorer, table):
    lib = _lib.load()
    z = lambda *shape, **kw: torch.zeros(shape, device=dev, **kw)   # noqa: E731
    S, L = 3, 50
    ok = dict(estimate=z(R, L), references=z(R, S, L), mixture=z(R, 2, L))
    scorer.score(spectral=True, **ok)
    gr, ge, gm, out = z(R, S, 1, L), z(R, 1, L), z(R, 2, L), z(R, 1, 1, 7, dtype=torch.float64)
    lag = z(R, 1, dtype=torch.int32)
    n0 = lib.m2h_launch_count()
    for tile in (7, 15999, 32000):
        with pytest.raises(ValueError, match="spectral=True needs tile = 16000 .*got %d" % tile):
            scorer.score(spectral=True, tile=tile, **ok)
    with pytest.raises(ValueError, match="mixture must live on cuda:0, got cpu"):
        scorer.score(spectral=True, **dict(ok, mixture=ok["mixture"].cpu()))
    with pytest.raises(RuntimeError, match=r"dft must be the \[32, 128, 2, 64\] table"):
        ops.score_spectral(gr, ge, gm, 0, table[:16])
    with pytest.raises(RuntimeError, match="with a lag"):
        ops.score_spectral(gr, ge, gm, 0, table, lag=None, D=4)
    with pytest.raises(RuntimeError, match="target = 3 is not one of the S = 3 references"):
        ops.score_spectral(gr, ge, gm, 3, table)

    def call(refs=gr, est=ge, mix=gm, target=None, target0=0, dft=table, res=out, nR=R, nS=S, nC=1, nL=L, lags=None, D=0):
        p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)   # noqa: E731
        return lib.m2h_score_spectral(p(refs), gr.stride(0), gr.stride(1), gr.stride(2), p(est), ge.stride(0), ge.stride(1), p(mix), gm.stride(0),
                                      gm.stride(1), p(target), target0, p(dft), p(res), nR, nS, nC, nL, p(lags), D, ctypes.c_void_p(0))

    refused = [dict(refs=None), dict(est=None), dict(mix=None), dict(dft=None), dict(res=None), dict(nS=0), dict(nS=7), dict(nC=0), dict(nC=3),
               dict(nR=0), dict(nL=0), dict(target0=-1), dict(target0=3), dict(D=4), dict(lags=lag), dict(lags=lag, D=8193),
               dict(lags=lag, D=25, nL=50), dict(nL=2 ** 31 * 16000)]
    for kw in refused:
        assert call(**kw) < 0, kw
    assert b"score_spectral" in lib.m2h_last_error()
    assert lib.m2h_launch_count() == n0
    assert call() == 0 and call(lags=lag, D=24, nL=50) == 0 and lib.m2h_launch_count() == n0 + 2
    torch.cuda.synchronize()


def test_cli_spectral_rows_and_json(dev, tmp_path):
    """score.py --spectral --json on small float32 WAVs: the new keys match the float64 definition within the bound and the printed rows
    parse; without the flag none of the new keys and none of the rows appear."""
    S, C, L = 2, 2, 20001
    refs, est, mix = (a[0, ..., :L] for a in batch(3, 2))
    refs = refs[:S]
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1")}
    for k, v in (("est", est), ("mix", mix), ("ref0", refs[0]), ("ref1", refs[1])):
        _write_wav(p[k], np.ascontiguousarray(v.T))
    out_json = str(tmp_path / "scores.json")
    cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"], "--reference", p["ref1"],
           "--json", out_json]
    run = lambda c: subprocess.run(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)   # noqa: E731
    res = run(cmd + ["--spectral"])
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    sums, bound = REF.recording_sums(refs, est, mix, 0)                                 # [C, J, 7]
    J = sums.shape[1]
    tsum, Q = REF.window_sums(sums)
    tbound, _ = REF.window_sums(bound)
    wsum, wbound = REF.window_sums(sums, J, 1)[0][:, 0], REF.window_sums(bound, J, 1)[0][:, 0]
    assert got["spectral_metrics"] == list(REF.ORDER) and np.array(got["spectral_track"]).shape == (C, J, 8)

    def check(values, s, b, q):
        """stft_l2, stft_l2_complex and their baselines within the bound that follows from the sums'; the improvements within the two
        bounds added; sc = sqrt(s3 / s0) moves by at most sc (b3 / s3 + b0 / s0) / 2 to first order: 1 % on top for the second"""
        values, want, mb = np.asarray(values), REF.metrics(s, q), REF.metrics_bound(s, b, q)
        tol = np.stack([mb[..., 0], mb[..., 1], 0.505 * want[..., 2] * (b[..., 3] / s[..., 3] + b[..., 0] / s[..., 0]), mb[..., 2], mb[..., 3],
                        0.505 * want[..., 5] * (b[..., 5] / s[..., 5] + b[..., 0] / s[..., 0]), mb[..., 0] + mb[..., 2], mb[..., 1] + mb[..., 3]], axis=-1)
        assert values.shape == want.shape and (np.abs(values - want) <= tol).all(), (values, want, tol)

    check(got["spectral_whole"], wsum, wbound, float(J))
    check(got["spectral_track"], tsum, tbound, Q)
    assert np.allclose(got["spectral_track_mean"], np.mean(got["spectral_track"], axis=1), rtol=1e-12, atol=0)
    assert np.allclose(got["spectral_track_median"], np.median(got["spectral_track"], axis=1), rtol=1e-12, atol=0)
    lines = res.stdout.splitlines()
    for c, name in enumerate(("left", "right")):
        for label, key in (("spectral whole", "spectral_whole"), ("spectral window mean", "spectral_track_mean"), ("spectral window median", "spectral_track_median")):
            row = [ln for ln in lines if ln.startswith("%-8s %-23s" % (name, label))]
            assert len(row) == 1, res.stdout
            assert np.allclose([float(v) for v in row[0][32:].split()], got[key][c], rtol=1e-11, atol=0), (name, label, row[0])
        for label in ("whole", "window mean", "window median"):                        # the existing rows: still one of each
            assert len([ln for ln in lines if ln.startswith("%-8s %-14s" % (name, label))]) == 1, res.stdout
    with_flag = got
    res = run(cmd)
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    assert not [k for k in got if k.startswith("spectral")]
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith("spectral") or "spectral w" in ln]
    assert json.dumps({k: v for k, v in with_flag.items() if not k.startswith("spectral")}) == json.dumps(got)
