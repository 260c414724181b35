"""STOI / ESTOI of the Scorer on the GPU (m2h/audio/score.py "STOI", csrc/score_stoi.hip) against tests/stoi_ref.py: the resampled signals
bit for bit against Resampler, the kept-frame mask and K exactly, the envelopes within the element bound, the segment kernel against step 3
on the kernel's own envelopes, Scorer.score(..., stoi=True) end to end, its bit-identical properties, alignment, no host synchronisation,
the Auralizer scenario and the command line.

Measured on an MI355X: see DESIGN.md §8.10 (worst envelope error / bound, the segment kernel against float64 and the float64-longdouble
spread, the six numbers against TOL_END_TO_END)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stoi_ref as REF
from score_cases import R, _gpu, _same, _target, _write_wav, recordings, targets
from m2h import ops
from m2h.audio import score as SC
from m2h.audio.resample import Resampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("stoi_whole", "stoi_track", "stoi_frames")
CASES = [(1, 1, 6000), (2, 3, 7000), (1, 3, 16000), (2, 1, 16001), (2, 3, 40001)]       # (C, S, L)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scorer(dev):
    return SC.Scorer(dev)


def batch(S, C, L):
    """R recordings of stoi_ref.inputs with a different target per recording: refs [R, S, C, L], est [R, C, L], mix [R, 2, L]"""
    tg = targets(S)
    return recordings(("stoi", S, C, L), lambda r: REF.inputs(L, 31 + 50 * r, S, C, target=tg[r])[:3])


def reference(S, C, L, window=1, hop=1):
    """stoi_ref.analyse_recording of every recording of batch(S, C, L), computed once per key (it asserts the mask margins)"""
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    return recordings(("stoi ref", S, C, L, window, hop),
                      lambda r: (lambda a: (a["six"], a["K"]))(REF.analyse_recording(refs[r], est[r], mix[r], tg[r], window=window, hop=hop)))


def hand_cut(gr, ge, gm, tg, lag=None, D=0):
    """[R, C, 3, Lr] contiguous: the three signals cut by hand with torch"""
    Rn, _, C, L = gr.shape
    rows = []
    for r in range(Rn):
        for c in range(C):
            s = 0 if lag is None else lag[r][c]
            b = gm[r, c, D:L - D] if C == 2 else 0.5 * (gm[r, 0, D:L - D] + gm[r, 1, D:L - D])
            rows += [gr[r, tg[r], c, D:L - D], ge[r, c, D + s:L - D + s], b]
    return torch.stack(rows).view(Rn, C, 3, L - 2 * D).contiguous()


@pytest.mark.parametrize("C,S,L", CASES)
def test_resample_is_bit_identical_to_the_resampler(dev, scorer, C, S, L):
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    table = scorer._stoi_tables()[0]
    rs = Resampler(16000, 10000, dev)
    assert torch.equal(table, rs.table) and tuple(table.shape) == (5, 33)
    got = ops.stoi_resample(gr, ge, gm, _target(dev, tg), table)
    assert ops.last_kernel() == "stoi_resample" and tuple(got.shape) == (R, C, 3, -(-L * 5 // 8))
    assert torch.equal(got, rs(hand_cut(gr, ge, gm, tg)))
    # the region [D, L - D) with the estimate at its lag, clamped to [-D, D], read from strided views at odd offsets
    D, lags = 64, [[37, 40][:C], [-5, 64][:C]]
    lag = torch.zeros((R, C), dtype=torch.int32, device=dev)
    for r in range(R):
        for c in range(C):
            lag[r, c].fill_(lags[r][c] if lags[r][c] != 64 else 900)                    # 900 is clamped to D = 64
    big = torch.zeros((R + 1, S + 1, C, L + 7), device=dev)
    big[1:, :S, :, 3:L + 3] = gr
    eb = torch.zeros((R, C + 1, L + 5), device=dev)
    eb[:, :C, 1:L + 1] = ge
    got = ops.stoi_resample(big[1:, :S, :, 3:L + 3], eb[:, :C, 1:L + 1], gm, _target(dev, tg), table, lag, D)
    assert torch.equal(got, rs(hand_cut(gr, ge, gm, tg, lags, D)))


@pytest.mark.parametrize("C,S,L", CASES)
def test_mask_envelopes_and_segments(dev, scorer, C, S, L):
    """Steps 1 .. 3 on the kernel's own 10 kHz signals: the kept frames and K exactly the reference's in every range, the envelopes within
    the element bound, the six numbers against step 3 of the reference on the kernel's own envelopes within 16 x the reference's own
    float64-longdouble spread on those envelopes."""
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    table, win, tw = scorer._stoi_tables()
    window = 2 if L > 32000 else 1
    plan = SC.score_plan(L, 16000, window, 1)
    sp = SC.stoi_plan(plan)
    x10 = ops.stoi_resample(gr, ge, gm, _target(dev, tg), table)
    st = ops.stoi_ranges(x10, scorer._stoi_ranges(plan, sp), sp["total"], win, tw)
    assert ops.last_kernel() == "stoi_ranges"
    torch.cuda.synchronize()
    assert scorer._stoi_ranges(plan, sp).cpu().tolist() == [[s, e, o] for (s, e), o in zip(sp["ranges"], sp["slots"])]
    hx, out, kept, lst, env = (t.cpu().numpy() for t in (x10, st["out"], st["kept"], st["list"], st["env"]))
    worst_env, spread, checks = 0.0, 0.0, []
    for r in range(R):
        for c in range(C):
            for q, ((s, e), off) in enumerate(zip(sp["ranges"], sp["slots"])):
                a = REF.analyse(hx[r, c, 0, s:e].astype(np.float64), [hx[r, c, 1, s:e].astype(np.float64), hx[r, c, 2, s:e].astype(np.float64)])
                K = a["K"]
                assert a["margin"] >= REF.MIN_MARGIN_DB and kept[r, c, q, 0] == K and kept[r, c, q, 1] == 0, (r, c, q, K, kept[r, c, q])
                assert np.array_equal(lst[r, c, off:off + K], np.nonzero(a["mask"])[0]), (r, c, q)
                if K < 2:
                    assert np.isnan(out[r, c, q]).all()
                    continue
                got_env = env[r, c, :, :, off:off + K - 1]
                assert got_env.shape == a["env"].shape
                worst_env = max(worst_env, REF.worst(got_env, a["env"], REF.env_bound(a)))
                want = np.array([REF.step3(got_env[0], got_env[p]) for p in (1, 2)])
                wide = np.array([REF.step3(got_env[0], got_env[p], dtype=np.longdouble) for p in (1, 2)])
                want6 = np.array([want[0, 0], want[0, 1], want[1, 0], want[1, 1], want[0, 0] - want[1, 0], want[0, 1] - want[1, 1]])
                assert np.array_equal(np.isnan(out[r, c, q]), np.isnan(want6)) and np.isnan(want6).all() == (K < 31), (r, c, q, K)
                if K >= 31:
                    spread = max(spread, float(np.abs(want - wide).max()))
                    checks.append(float(np.abs(out[r, c, q] - want6).max()))
    worst_seg = max(checks) if checks else 0.0
    print("stoi C = %d, S = %d, L = %d: envelopes worst error / bound %.3e; segments worst |kernel - float64| %.3e, float64-longdouble spread %.3e (x 16 = %.3e)"
          % (C, S, L, worst_env, worst_seg, spread, 16 * spread))
    assert worst_env <= 1.0
    assert worst_seg <= 16 * spread


@pytest.mark.parametrize("C,S,L", CASES)
@pytest.mark.parametrize("window,hop", [(1, 1), (2, 1)])
def test_six_numbers_end_to_end(dev, scorer, C, S, L, window, hop):
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    want, K = reference(S, C, L, window, hop)                                           # [R, C, 1 + M, 6], [R, C, 1 + M]
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, window=window, hop=hop, stoi=True)
    M = res["plan"]["M"]
    assert res["stoi_whole"].dtype == torch.float64 and tuple(res["stoi_whole"].shape) == (R, C, 6)
    assert res["stoi_track"].dtype == torch.float64 and tuple(res["stoi_track"].shape) == (R, C, M, 6)
    assert res["stoi_frames"].dtype == torch.int64 and tuple(res["stoi_frames"].shape) == (R, C, 1 + M)
    got = torch.cat([res["stoi_whole"][:, :, None], res["stoi_track"]], dim=2).cpu().numpy()
    assert np.array_equal(res["stoi_frames"].cpu().numpy(), K)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want[:, :, 0]).all() == (L < 16000)
    d = float(np.nanmax(np.abs(got - want))) if not np.isnan(want).all() else 0.0
    print("stoi end to end C = %d, S = %d, L = %d, window %d: worst |difference| %.3e of %.3e" % (C, S, L, window, d, REF.TOL_END_TO_END))
    assert d <= REF.TOL_END_TO_END


def test_batch_slices_strides_and_other_keys_are_bit_identical(dev, scorer):
    C, S, L = 2, 3, 40001
    refs, est, mix = batch(S, C, L)
    tg = targets(S)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    res = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, stoi=True)
    # each recording of the batch against its solo call
    for r in range(R):
        solo = scorer.score(ge[r:r + 1].contiguous(), gr[r:r + 1].contiguous(), gm[r:r + 1].contiguous(), target=tg[r], window=2, hop=1, stoi=True)
        assert all(_same(solo[k][0], res[k][r]) for k in KEYS)
    # track[m] against that slice of the 10 kHz signals scored whole, read in place
    table, win, tw = scorer._stoi_tables()
    x10 = ops.stoi_resample(gr, ge, gm, _target(dev, tg), table)
    sp = SC.stoi_plan(res["plan"])
    for m, (s, e) in enumerate(sp["ranges"][1:]):
        whole = torch.tensor([[0, e - s, 0]], dtype=torch.int64).to(dev)                # one range: the whole slice
        alone = ops.stoi_ranges(x10[..., s:e], whole, max(1, SC.stoi_frames(e - s)), win, tw)
        assert _same(alone["out"][:, :, 0], res["stoi_track"][:, :, m]) and torch.equal(alone["kept"][:, :, 0, 0], res["stoi_frames"][:, :, 1 + m].int()), m
    # strided views inside larger buffers, and rows at odd element offsets against rows that are all 16-byte aligned
    images = torch.zeros((R + 1, S + 2, C, L + 9), device=dev)
    images[1:, 1:S + 1, :, 5:L + 5] = gr
    big = torch.zeros((R, 3, L + 3), device=dev)
    big[:, 1:, 2:L + 2] = ge
    mixbuf = torch.zeros((R, 2, 2 * L), device=dev)
    mixbuf[:, :, L - 1:2 * L - 1] = gm
    views = (big[:, 1:, 2:L + 2], images[1:, 1:S + 1, :, 5:L + 5], mixbuf[:, :, L - 1:2 * L - 1])
    assert not any(v.is_contiguous() for v in views)
    strided = scorer.score(*views, target=tg, window=2, hop=1, stoi=True)
    assert all(_same(strided[k], res[k]) for k in KEYS)
    assert L % 4 == 1 and all(t.data_ptr() % 16 == 0 for t in (gr, ge, gm))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (3,), device=dev)], dim=-1)[..., :L]   # noqa: E731  (row stride L + 3)
    aligned = scorer.score(pad(ge), pad(gr), pad(gm), target=tg, window=2, hop=1, stoi=True)
    assert all(_same(aligned[k], res[k]) for k in KEYS)
    # every other key with and without stoi=True, composed with align, spectral and spatial
    for kw in (dict(), dict(spectral=True, spatial=True), dict(align=16, spectral=True, spatial=True)):
        without = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, **kw)
        with_stoi = scorer.score(ge, gr, gm, target=tg, window=2, hop=1, stoi=True, **kw)
        assert not any(k in without for k in KEYS) and set(with_stoi) == set(without) | set(KEYS)
        for k, v in without.items():
            assert with_stoi[k] == v if k == "plan" else (_same(with_stoi[k], v) if v.dtype.is_floating_point else torch.equal(with_stoi[k], v)), (kw, k)
        if "align" not in kw:
            assert all(_same(with_stoi[k], res[k]) for k in KEYS)


def test_alignment_reads_each_ear_at_its_own_lag(dev, scorer):
    """align=64 on an estimate that is the target late by 37 samples in the left ear and 40 in the right: the same bits as slices cut by hand
    at those lags and scored without align."""
    D, lags, S, C = 64, [37, 40], 3, 2
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
    res = scorer.score(ge, gr, gm, target=tg, align=D, stoi=True)
    assert res["lag"].cpu().tolist() == [lags] * R
    cut_est = torch.stack([ge[:, c, D + lags[c]:L - D + lags[c]] for c in range(C)], dim=1)
    cut = scorer.score(cut_est, gr[..., D:L - D], gm[..., D:L - D], target=tg, stoi=True)
    assert all(_same(res[k], cut[k]) for k in KEYS)
    assert res["plan"]["J"] == 2 and tuple(res["stoi_track"].shape) == (R, C, 2, 6) and bool((res["stoi_whole"][..., 0] > 0.99).all())


def test_stoi_path_makes_no_host_synchronisation(dev, scorer):
    refs, est, mix = batch(3, 2, 40001)
    gr, ge, gm = _gpu(dev, refs, est, mix)
    want = scorer.score(ge, gr, gm, target=[0, 1], window=2, stoi=True)
    aligned = scorer.score(ge, gr, gm, target=[0, 1], window=2, align=16, stoi=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = scorer.score(ge, gr, gm, target=[0, 1], window=2, stoi=True)
        res16 = scorer.score(ge, gr, gm, target=[0, 1], window=2, align=16, stoi=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(_same(res[k], want[k]) for k in KEYS) and all(_same(res16[k], aligned[k]) for k in KEYS)


def test_argument_errors_launch_nothing(dev, scorer):
    from m2h import _lib
    lib = _lib.load()
    z = lambda *shape, **kw: torch.zeros(shape, device=dev, **kw)   # noqa: E731
    ok = dict(estimate=z(R, 50), references=z(R, 3, 50), mixture=z(R, 2, 50))
    assert bool(torch.isnan(scorer.score(stoi=True, **ok)["stoi_whole"]).all())         # digital silence, and too short: NaN
    n0 = lib.m2h_launch_count()
    for tile in (7, 15999, 32000):
        with pytest.raises(ValueError, match="stoi=True needs tile = 16000 .*got %d" % tile):
            scorer.score(stoi=True, tile=tile, **ok)
    with pytest.raises(ValueError, match="mixture must live on cuda:0, got cpu"):
        scorer.score(stoi=True, **dict(ok, mixture=ok["mixture"].cpu()))
    table, win, tw = scorer._stoi_tables()
    with pytest.raises(RuntimeError, match=r"table must be the \[5, 33\] table"):
        ops.stoi_resample(z(R, 3, 1, 50), z(R, 1, 50), z(R, 2, 50), 0, table[:4])
    with pytest.raises(RuntimeError, match="with a lag"):
        ops.stoi_resample(z(R, 3, 1, 50), z(R, 1, 50), z(R, 2, 50), 0, table, lag=None, D=4)
    with pytest.raises(RuntimeError, match="unit stride and lie a constant distance apart"):
        ops.stoi_ranges(z(R, 2, 3, 40)[:, :, :, ::2], z(1, 3, dtype=torch.int64), 1, win, tw)
    assert lib.m2h_launch_count() == n0


def test_scenario_auralizer_scorer(dev, scorer):
    """Auralizer.render(..., return_images=True) of two sources: the target image as the estimate is perfectly intelligible and better than
    the mixture; the mixture as the estimate is exactly as intelligible as the baseline."""
    from m2h.audio.render import Auralizer
    L, Lr = 40000, 96
    rng = np.random.default_rng(3)
    t = np.arange(L) / 16000.0
    src = np.stack([np.stack([0.3 * rng.standard_normal(L) * (1 + 0.9 * np.sin(2 * np.pi * (2.7 + s + r) * t)) for s in range(2)]) for r in range(R)])
    rirs = rng.standard_normal((R, 2, Lr, 2)) * np.exp(-np.arange(Lr) / 20.0)[None, None, :, None]
    xs, hs = _gpu(dev, src.astype(np.float32), rirs.astype(np.float32))
    mix, images = Auralizer(dev).render(xs, hs, return_images=True)
    refs = 0.5 * images                                                                 # the sources as they are in the mixture (gains 1 / S)
    same = scorer.score(refs[:, 0].contiguous(), refs, mix, stoi=True)
    for key in ("stoi_whole", "stoi_track"):
        v = same[key]
        assert bool(((v[..., :2] - 1).abs() <= REF.TOL_END_TO_END).all()) and bool((v[..., 4:] > 0).all()), (key, v)
    base = scorer.score(mix, refs, mix, stoi=True)
    for key in ("stoi_whole", "stoi_track"):
        assert bool((base[key][..., 4:] == 0).all()) and bool(torch.equal(base[key][..., :2], base[key][..., 2:4]))


def test_cli_stoi_rows_and_json(dev, tmp_path):
    """score.py --stoi --json on float32 WAVs of 20001 samples against stoi_ref; without the flag no stoi key or row, the rest byte-equal."""
    S, C, L = 2, 2, 20001
    refs, est, mix, tg = REF.inputs(L, 77, S, C, target=0)
    p = {k: str(tmp_path / (k + ".wav")) for k in ("est", "mix", "ref0", "ref1")}
    for k, v in (("est", est), ("mix", mix), ("ref0", refs[0]), ("ref1", refs[1])):
        _write_wav(p[k], np.ascontiguousarray(v.T))
    out_json = str(tmp_path / "scores.json")
    cmd = [sys.executable, os.path.join(ROOT, "score.py"), "--estimate", p["est"], "--mixture", p["mix"], "--reference", p["ref0"], "--reference", p["ref1"],
           "--json", out_json]
    run = lambda c: subprocess.run(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)   # noqa: E731
    res = run(cmd + ["--stoi"])
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    a = REF.analyse_recording(refs, est, mix, 0)
    assert got["stoi_metrics"] == list(REF.ORDER) and got["stoi_frames"] == a["K"].tolist()
    whole, track = np.array(got["stoi_whole"]), np.array(got["stoi_track"], dtype=np.float64)
    assert track.shape == (C, 2, 6) and np.abs(whole - a["six"][:, 0]).max() <= REF.TOL_END_TO_END
    assert np.array_equal(np.isnan(track), np.isnan(a["six"][:, 1:])) and np.isnan(track[:, 1]).all() and not np.isnan(track[:, 0]).any()
    assert np.abs(track[:, 0] - a["six"][:, 1]).max() <= REF.TOL_END_TO_END
    assert np.allclose(got["stoi_track_mean"], track[:, 0], rtol=1e-12, atol=0) and np.allclose(got["stoi_track_median"], track[:, 0], rtol=1e-12, atol=0)
    lines = res.stdout.splitlines()
    for c, name in enumerate(("left", "right")):
        for label, key in (("stoi whole", "stoi_whole"), ("stoi window mean", "stoi_track_mean"), ("stoi window median", "stoi_track_median")):
            row = [ln for ln in lines if ln.startswith("%-8s %-23s" % (name, label))]
            assert len(row) == 1, res.stdout
            assert np.allclose([float(v) for v in row[0][32:].split()], got[key][c], rtol=1e-11, atol=0), (name, label, row[0])
    with_flag, with_lines = got, lines
    res = run(cmd)
    assert res.returncode == 0, res.stdout
    got = json.load(open(out_json))
    assert not [k for k in got if k.startswith("stoi")]
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith("stoi") or "stoi w" in ln]
    assert json.dumps({k: v for k, v in with_flag.items() if not k.startswith("stoi")}) == json.dumps(got)
    assert [ln for ln in with_lines if not (ln.startswith("stoi") or "stoi w" in ln)] == res.stdout.splitlines()
