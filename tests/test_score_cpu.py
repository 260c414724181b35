"""CPU: the Scorer's algebra (m2h.audio.score.metrics_from_gram on a float64 Gram) against the direct float64 definition
(tests/score_ref.py), what the 1e-9 dB bound rejects, the degenerate cases, score_plan, and every argument error that needs no GPU.

Measured on the CPU, largest error of any compared metric in dB: 5.3e-12 at S = 3, L = 40001 (about 12 dB SI-SDR) and 3.5e-10 on the
43 dB estimate; the same Gram accumulated in fp32 misses by 1.7e-4 and 5.4e-2.
"""
import ctypes

import numpy as np
import pytest
import torch

import score_ref as REF
from m2h import _lib
from m2h.audio import score as SC

CASES = [(1, 16000, False), (2, 15999, False), (3, 40001, False), (3, 5, False), (6, 40001, False), (3, 40001, True)]
TILE = 16000


def _metrics(gram, n, target=0, C=1):
    """gram [C, M, K] numpy, n [M] -> [C, M, 11] numpy through metrics_from_gram (R = 1)"""
    g = torch.from_numpy(np.ascontiguousarray(gram))[None]
    out = SC.metrics_from_gram(g, torch.as_tensor(np.asarray(n, np.float64)), target, C)
    assert out.dtype == torch.float64 and tuple(out.shape) == g.shape[:-1] + (11,)
    return out[0].numpy()


def _windows(L, tile=TILE):
    return [(0, L)] + REF.plan_windows(L, tile)


@pytest.mark.parametrize("S,L,snr43", CASES)
def test_gram_algebra_equals_the_direct_float64_scores(S, L, snr43):
    refs, est, mix = REF.inputs(S, L, 7 + S, snr43=snr43)
    wins = _windows(L)
    got = _metrics(REF.gram_recording(refs, est, mix, wins), [b - a for a, b in wins])
    whole, track = REF.score_direct_f64(refs, est, mix, tile=TILE)
    want = np.concatenate([whole[:, None], track], axis=1)
    cols = REF.WELL if S == 1 else REF.ALL
    err = REF.max_err(got, want, cols)
    print("S=%d L=%d snr43=%s: si_sdr %.2f dB, largest error %.3e dB" % (S, L, snr43, want[0, 0, 0], err))
    assert np.isfinite(want[..., list(cols)]).all()
    assert err <= REF.TOL_ALGEBRA
    if snr43:
        assert 40.0 < want[0, 0, 0] < 46.0


def test_two_channels_and_another_target():
    refs, est, mix = REF.inputs(3, 20001, 5, C=2)
    est = (0.8 * refs[2] + 0.05 * refs[0] + 0.03 * np.random.default_rng(1).standard_normal(est.shape)).astype(np.float32)   # (artefacts: SI-SAR is not rounding noise)
    wins = _windows(20001)
    got = _metrics(REF.gram_recording(refs, est, mix, wins), [b - a for a, b in wins], target=2, C=2)
    whole, track = REF.score_direct_f64(refs, est, mix, target=2, tile=TILE)
    assert REF.max_err(got, np.concatenate([whole[:, None], track], axis=1)) <= REF.TOL_ALGEBRA
    # per-recording targets: the same numbers as one call per target
    g = torch.from_numpy(REF.gram_recording(refs, est, mix, wins))
    both = SC.metrics_from_gram(torch.stack([g, g]), torch.tensor([float(b - a) for a, b in wins]), torch.tensor([2, 0]), 2)
    assert torch.equal(both[0], torch.from_numpy(got)) and REF.max_err(both[1].numpy(), _metrics(g.numpy(), [b - a for a, b in wins], 0, 2)) == 0.0


def test_what_the_bound_rejects():
    """Each defective scorer misses the direct scores by more than 1e-6 dB on every metric it affects (S = 3, L = 40001)."""
    S, L = 3, 40001
    refs, est, mix = REF.inputs(S, L, 10)
    N = S + 3
    whole, track = REF.score_direct_f64(refs, est, mix, tile=TILE)

    def smallest(got, want, cols):
        return float(np.abs(np.asarray(got)[..., list(cols)] - np.asarray(want)[..., list(cols)]).min())

    g_whole = REF.gram_recording(refs, est, mix, [(0, L)])
    assert REF.max_err(_metrics(g_whole, [L]), whole[:, None]) <= REF.TOL_ALGEBRA
    # means not removed
    g = g_whole.copy()
    g[..., :N] = 0.0
    e1 = smallest(_metrics(g, [L]), whole[:, None], REF.WELL)
    # baseline taken from the left channel alone: only the improvements move
    e2 = smallest(_metrics(REF.gram_recording(refs, est, np.stack([mix[0], mix[0]]), [(0, L)]), [L]), whole[:, None], (6, 7, 8))
    # last, short tile dropped
    e3 = smallest(_metrics(REF.gram_recording(refs, est, mix, [(0, 32000)]), [32000]), whole[:, None], REF.WELL)
    # the whole recording's means used inside a window
    f = lambda a: (np.asarray(a, np.float64) - np.asarray(a, np.float64).mean(axis=-1, keepdims=True))   # noqa: E731
    g = REF.gram_recording(f(refs), f(est), f(mix), [(16000, 32000)])
    g[..., :N] = 0.0
    e4 = smallest(_metrics(g, [16000]), track[:, 1:2], REF.WELL)
    print("defects: no means %.3e, left baseline %.3e, tile dropped %.3e, global means %.3e dB" % (e1, e2, e3, e4))
    assert min(e1, e2, e3, e4) > REF.TOL_DEFECT


def test_an_fp32_gram_is_not_enough():
    """The same Gram accumulated in fp32 misses the 43 dB case by far more than the GPU bound."""
    refs, est, mix = REF.inputs(3, 40001, 10, snr43=True)
    whole, _ = REF.score_direct_f64(refs, est, mix, tile=TILE)
    rows = REF.gram_rows(refs, est, mix, 0, 0, 40001, np.float32)
    N = len(rows)
    A = np.stack(rows)
    G32 = A @ A.T
    g = np.array([a.sum(dtype=np.float32) for a in rows] + [G32[i, k] for i in range(N) for k in range(i, N)], np.float64)
    err = REF.max_err(_metrics(g[None, None], [40001]), whole[:, None], REF.WELL)
    print("fp32 Gram, 43 dB case: %.3e dB" % err)
    assert err > 10 * REF.TOL_GPU


def test_degenerate_cases():
    S, L = 3, 4000
    refs, est, mix = REF.inputs(S, L, 3)
    one = lambda r, e, m, n=L: _metrics(REF.gram_recording(r, e, m, [(0, n)]), [n])[0, 0]   # noqa: E731
    # a silent interferer is left out of the projection
    quiet = refs.copy()
    quiet[1] = 0.0
    want = REF.score_window_direct(quiet, est, mix, 0, 0, 0, L)
    assert np.isfinite(want).all() and REF.max_err(one(quiet, est, mix), want) <= REF.TOL_ALGEBRA
    assert REF.max_err(one(quiet, est, mix), REF.score_window_direct(quiet[[0, 2]], est, mix, 0, 0, 0, L)) <= REF.TOL_ALGEBRA
    # a silent target, n = 1: all NaN
    dead = refs.copy()
    dead[0] = 0.0
    assert np.isnan(one(dead, est, mix)).all() and np.isnan(REF.score_window_direct(dead, est, mix, 0, 0, 0, L)).all()
    assert np.isnan(one(refs, est, mix, 1)).all() and np.isnan(REF.score_window_direct(refs, est, mix, 0, 0, 0, 1)).all()
    assert np.isnan(_metrics(np.zeros((1, 1, 27)), [0])).all()                    # an empty window
    assert REF.max_err(one(refs, est, mix, 3), REF.score_window_direct(refs, est, mix, 0, 0, 0, 3), REF.WELL) <= REF.TOL_ALGEBRA    # n = 3 is scored
    # duplicate references: the normal equations cannot be solved; SIR / SAR and their improvements are NaN, the rest stands
    dup = refs.copy()
    dup[2] = dup[1]
    got, want = one(dup, est, mix), REF.score_window_direct(refs[:1], est, mix, 0, 0, 0, L)
    assert np.isnan(got[[1, 2, 9, 10]]).all() and REF.max_err(got, want, REF.WELL) <= REF.TOL_ALGEBRA
    # an exact scaled copy of the target scores +inf, not NaN
    got = one(refs, 0.5 * refs[0], mix)
    assert got[0] == np.inf and got[6] == np.inf and not np.isnan(got[:6]).any() and abs(got[5] - 0.0) < 1e-12   # srr of alpha = 1/2: 0 dB
    got = one(refs, refs[0], mix)
    assert got[0] == np.inf and got[4] == np.inf and got[5] == np.inf and not np.isnan(got[:6]).any()


def test_score_plan():
    p = SC.score_plan(40001, 16000, 1, 1)
    assert (p["J"], p["M"]) == (3, 3) and p["tiles"] == [(0, 1), (1, 2), (2, 3)] and p["samples"][-1] == (32000, 40001)
    assert p["samples"] == REF.plan_windows(40001, 16000)
    p = SC.score_plan(40001, 16000, 5, 2)                                         # J <= w: one window, the whole recording
    assert p["M"] == 1 and p["tiles"] == [(0, 3)] and p["samples"] == [(0, 40001)]
    p = SC.score_plan(16000 * 3, 16000, 3, 1)
    assert p["M"] == 1 and p["samples"] == [(0, 48000)]
    p = SC.score_plan(16000 * 6 + 1, 16000, 3, 2)                                 # J = 7: a short last window
    assert p["J"] == 7 and p["M"] == 3 and p["tiles"] == [(0, 3), (2, 5), (4, 7)] and p["samples"][-1] == (64000, 96001)
    p = SC.score_plan(16000 * 6, 16000, 3, 2)                                     # J = 6: the last window is cut to two tiles
    assert p["M"] == 3 and p["tiles"][-1] == (4, 6)
    p = SC.score_plan(70, 7, 2, 5)                                                # h > w: tiles left out, and an empty last window
    assert p["J"] == 10 and p["M"] == 3 and p["tiles"] == [(0, 2), (5, 7), (10, 10)] and p["samples"][-1] == (70, 70)
    assert p["samples"] == REF.plan_windows(70, 7, 2, 5)
    assert SC.score_plan(1)["samples"] == [(0, 1)]
    for bad in (dict(L=0), dict(tile=0), dict(window=0), dict(hop=-1)):
        with pytest.raises(ValueError, match=r"%s must be at least 1, got %d" % list(bad.items())[0]):
            SC.score_plan(**dict(dict(L=100), **bad))
    with pytest.raises(TypeError, match="tile must be an int"):
        SC.score_plan(100, 16000.0)


def test_kernel_argument_errors_need_no_gpu():
    """Every argument error of m2h_score_gram (and m2h_score_windows): a negative status, a message, nothing launched."""
    lib = _lib.load()
    p = ctypes.c_void_p(256)          # never dereferenced: the call fails before any launch
    n0 = lib.m2h_launch_count()

    def gram(refs=p, est=p, mix=p, out=p, R=2, S=3, C=1, L=100, tile=10):
        return lib.m2h_score_gram(refs, 300, 100, 0, est, 100, 0, mix, 200, 100, out, R, S, C, L, tile, None)

    for kw, text in ((dict(refs=None), b"null pointer"), (dict(est=None), b"null pointer"), (dict(mix=None), b"null pointer"),
                     (dict(out=None), b"null pointer"), (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(C=0), b"C = 0"), (dict(C=3), b"C = 3"),
                     (dict(L=0), b"L = 0"), (dict(tile=0), b"tile = 0"), (dict(R=0), b"R = 0"), (dict(R=1 << 20, L=1 << 40, tile=1), b"exceed a grid")):
        assert gram(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert b"score_gram" in msg and text in msg, (kw, msg)
    for args in ((None, p, 1, 1, 9, 1, 1, 1), (p, None, 1, 1, 9, 1, 1, 1), (p, p, 0, 1, 9, 1, 1, 1), (p, p, 1, 0, 9, 1, 1, 1), (p, p, 1, 1, 0, 1, 1, 1),
                 (p, p, 1, 1, 9, 0, 1, 1), (p, p, 1, 1, 9, 1, 0, 1), (p, p, 1, 1, 9, 1, 1, 0)):
        assert lib.m2h_score_windows(*args, None) < 0 and b"score_windows" in lib.m2h_last_error(), args
    assert lib.m2h_launch_count() == n0


def test_metrics_from_gram_argument_errors():
    g = torch.zeros((1, 1, 1, 27), dtype=torch.float64)
    with pytest.raises(TypeError, match="float64"):
        SC.metrics_from_gram(g.float(), 10, 0, 1)
    with pytest.raises(ValueError, match="not 26"):
        SC.metrics_from_gram(g[..., :26], 10, 0, 1)
    with pytest.raises(ValueError, match=r"C = 2"):
        SC.metrics_from_gram(g, 10, 0, 2)
    with pytest.raises(ValueError, match="target = 3"):
        SC.metrics_from_gram(g, 10, 3, 1)
    with pytest.raises(TypeError, match="tensor `target`"):
        SC.metrics_from_gram(g, 10, torch.tensor([0.0]), 1)


def scorer_argument_errors(dev):
    """(exception, message pattern, keyword arguments) for every argument error of Scorer.score, on tensors of device `dev`"""
    z = lambda *shape, **kw: torch.zeros(shape, device=dev, **kw)   # noqa: E731
    R, S, L = 2, 3, 50
    ok = dict(estimate=z(R, L), references=z(R, S, L), mixture=z(R, 2, L))
    bad = [
        (TypeError, "estimate must be a torch tensor", dict(estimate=np.zeros((R, L), np.float32))),
        (TypeError, "references must be float32, got torch.float64", dict(references=z(R, S, L, dtype=torch.float64))),
        (TypeError, "mixture must be float32, got torch.float16", dict(mixture=z(R, 2, L, dtype=torch.float16))),
        (ValueError, r"references must be \[R, S, L\] or \[R, S, C, L\], got a tensor of shape \(2, 50\)", dict(references=z(R, L))),
        (ValueError, r"estimate must be \[R, L\] or \[R, C, L\], got a tensor of shape \(50,\)", dict(estimate=z(L))),
        (ValueError, r"mixture must be \[R, 2, L\], got a tensor of shape \(2, 1, 50\)", dict(mixture=z(R, 1, L))),
        (ValueError, "C = 3 channels", dict(references=z(R, S, 3, L), estimate=z(R, 3, L))),
        (ValueError, "references have C = 2 channels and the estimate has 1", dict(references=z(R, S, 2, L))),
        (ValueError, "references have C = 1 channels and the estimate has 2", dict(estimate=z(R, 2, L))),
        (ValueError, "S = 7 reference sources", dict(references=z(R, 7, L))),
        (ValueError, "S = 0 reference sources", dict(references=z(R, 0, L))),
        (ValueError, "R = 2, 3 and 2 recordings", dict(estimate=z(3, L))),
        (ValueError, "R = 2, 2 and 1 recordings", dict(mixture=z(1, 2, L))),
        (ValueError, "L = 50, 49 and 50 samples", dict(estimate=z(R, L - 1))),
        (ValueError, "L = 50, 50 and 51 samples", dict(mixture=z(R, 2, L + 1))),
        (ValueError, "L = 0, 0 and 0 samples", dict(estimate=z(R, 0), references=z(R, S, 0), mixture=z(R, 2, 0))),
        (ValueError, "last stride of estimate is 2", dict(estimate=z(R, 2 * L)[:, ::2])),
        (ValueError, "last stride of references is 3", dict(references=z(R, S, 3 * L)[..., ::3])),
        (ValueError, "last stride of mixture is 2", dict(mixture=z(R, L, 2).transpose(1, 2)[:, :, :L])),
        (ValueError, "target 3 is not one of the S = 3 references", dict(target=3)),
        (ValueError, "target -1 is not", dict(target=[0, -1])),
        (ValueError, "R = 2 ints, got 3 of them", dict(target=[0, 1, 2])),
        (TypeError, "target must be an int or R ints, got 0.5", dict(target=0.5)),
        (TypeError, "target must be an int or R ints", dict(target=[0, 1.5])),
        (ValueError, "tile must be at least 1, got 0", dict(tile=0)),
        (ValueError, "window must be at least 1, got 0", dict(window=0)),
        (ValueError, "hop must be at least 1, got -2", dict(hop=-2)),
        (TypeError, "window must be an int", dict(window=1.5)),
    ]
    return ok, bad


def test_scorer_argument_errors():
    """Every argument error of Scorer.score is raised before the device is touched: shapes, strides and targets are checked on host
    tensors here; with everything else in order a host tensor is refused by name."""
    sc = SC.Scorer(torch.device("cuda", 0))
    ok, bad = scorer_argument_errors("cpu")
    for exc, pattern, kw in bad:
        with pytest.raises(exc, match=pattern):
            sc.score(**dict(ok, **kw))
    with pytest.raises(ValueError, match="estimate must live on cuda:0, got cpu"):
        sc.score(**ok)


def test_solve_pivoted_is_solve_ex_and_ignores_the_batch():
    g = torch.Generator().manual_seed(3)
    for S in (1, 2, 3, 6):
        A = torch.randn((40, S, S), generator=g, dtype=torch.float64)
        A[:20] = A[:20] @ A[:20].transpose(1, 2)                                  # Gram matrices, and general ones that need their pivots
        Y = torch.randn((40, S, 2), generator=g, dtype=torch.float64)
        X, singular = SC.solve_pivoted(A, Y)
        want, info = torch.linalg.solve_ex(A, Y)
        assert not bool(singular.any()) and bool((info == 0).all())
        assert float((X - want).abs().max() / want.abs().max()) < 1e-9
        for i in (0, 7, 39):                                                      # alone, and inside another batch: bit for bit
            assert torch.equal(SC.solve_pivoted(A[i:i + 1], Y[i:i + 1])[0][0], X[i])
            assert torch.equal(SC.solve_pivoted(A[i:].reshape(-1, 1, S, S), Y[i:].reshape(-1, 1, S, 2))[0][0, 0], X[i])
    A = torch.tensor([[2.0, 2.0, 1.0], [2.0, 2.0, 1.0], [1.0, 1.0, 3.0]], dtype=torch.float64)     # duplicate references
    _, singular = SC.solve_pivoted(A[None], torch.ones((1, 3, 1), dtype=torch.float64))
    assert bool(singular[0]) and int(torch.linalg.solve_ex(A, torch.ones((3, 1), dtype=torch.float64))[1]) != 0
