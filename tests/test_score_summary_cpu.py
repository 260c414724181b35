"""CPU: m2h.audio.score.summarize on a synthetic result of every metric family against a direct numpy restatement written here.

The restatement uses the same numpy reductions (mean and median along axis 0 of the kept rows) on the same float64 values, so every
number is compared for equality, NaN in the same places.  R = 2 recordings, C = 2 channels, M = 5 windows: recording 0 has a window that
is active in one ear only and one that is active in neither; recording 1 has no active window at all; the STOI track has rows that are
NaN throughout and one with a single NaN.
"""
import numpy as np
import torch

from m2h.audio import score as SC

R, C, M = 2, 2, 5
ACTIVE = np.array([[[True, True, False, True, True], [True, False, False, True, True]],
                   [[False] * M, [False] * M]])
# (prefix, order, per recording instead of per channel)
FAMILIES = (("", SC.METRIC_ORDER, False), ("spectral_", SC.SPECTRAL_ORDER, False), ("spatial_", SC.SPATIAL_ORDER, True),
            ("itd_", SC.ITD_ORDER, True), ("stoi_", SC.STOI_ORDER, False), ("bss_", SC.BSS_ORDER, False))
KEYS = ["metrics", "whole", "track_mean", "track_median", "active_windows",
        "spectral_metrics", "spectral_whole", "spectral_track_mean", "spectral_track_median",
        "spatial_metrics", "spatial_whole", "spatial_track_mean", "spatial_track_median",
        "itd_metrics", "itd_whole", "itd_track_mean", "itd_track_median",
        "stoi_metrics", "stoi_whole", "stoi_track_mean", "stoi_track_median", "stoi_frames",
        "bss_metrics", "bss_whole", "bss_track_mean", "bss_track_median"]


def _result():
    """a result dict as Scorer.score returns it with every option on, of CPU float64 tensors"""
    rng = np.random.default_rng(3)
    res = {}
    for prefix, order, binaural in FAMILIES:
        lead = (R,) if binaural else (R, C)
        res[prefix + "whole"] = rng.standard_normal(lead + (len(order),))
        res[prefix + "track"] = rng.standard_normal(lead + (M, len(order)))
    res["track"][0, 0, 2] = np.nan                                                      # an inactive window's row is NaN and must not enter
    res["stoi_track"][0, 0, 1] = np.nan                                                 # a window without STOI
    res["stoi_track"][0, 1, 3, 4] = np.nan                                              # one NaN is enough to leave the row out
    res["stoi_track"][1, 1] = np.nan                                                    # a channel without any
    res = {k: torch.from_numpy(v) for k, v in res.items()}
    res["active"] = torch.from_numpy(ACTIVE)
    res["spatial_cues"] = torch.from_numpy(rng.standard_normal((R, M, 3, 32, 3)))
    res["itd_gcc"] = torch.from_numpy(rng.standard_normal((R, 1 + M, 3, 257)))
    res["stoi_frames"] = torch.from_numpy(rng.integers(0, 80, (R, C, 1 + M)))
    res["plan"] = SC.score_plan(5 * 16000)
    return res


def _stats(rows):
    """mean and median of the kept rows [n, K]; NaN without any"""
    if rows.shape[0] == 0:
        return [np.full(rows.shape[1], np.nan)] * 2
    return rows.mean(axis=0), np.median(rows, axis=0)


def _same(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def test_summarize_against_a_numpy_restatement_key_by_key():
    res = _result()
    s = SC.summarize(res)
    assert list(s) == KEYS
    assert s["active_windows"] == [[4, 3], [0, 0]]
    assert s["stoi_frames"] == res["stoi_frames"].tolist()
    for prefix, order, binaural in FAMILIES:
        whole, track = res[prefix + "whole"].numpy(), res[prefix + "track"].numpy()
        assert s[prefix + "metrics"] == list(order)
        assert _same(s[prefix + "whole"], whole), prefix
        mean, median = np.array(s[prefix + "track_mean"]), np.array(s[prefix + "track_median"])
        assert mean.shape == median.shape == whole.shape, prefix
        for r in range(R):
            if binaural:                                                                # the windows active in both ears
                want = _stats(track[r][ACTIVE[r, 0] & ACTIVE[r, 1]])
                assert _same(mean[r], want[0]) and _same(median[r], want[1]), (prefix, r)
                continue
            for c in range(C):
                if prefix == "stoi_":                                                   # the windows whose rows hold no NaN
                    keep = np.array([not np.isnan(track[r, c, m]).any() for m in range(M)])
                else:                                                                   # the active windows
                    keep = ACTIVE[r, c]
                want = _stats(track[r, c][keep])
                assert _same(mean[r, c], want[0]) and _same(median[r, c], want[1]), (prefix, r, c)
    # what the rules come to on this input
    assert np.isnan(s["track_mean"][1]).all() and np.isnan(s["spatial_track_median"][1]).all() and np.isnan(s["stoi_track_mean"][1][1]).all()
    assert not np.isnan(s["track_mean"][0]).any() and not np.isnan(s["stoi_track_mean"][0]).any() and not np.isnan(s["stoi_track_mean"][1][0]).any()
    assert _same(s["itd_track_mean"][0], res["itd_track"].numpy()[0][[0, 3, 4]].mean(axis=0))
    assert _same(s["stoi_track_median"][0][1], np.median(res["stoi_track"].numpy()[0, 1][[0, 1, 2, 4]], axis=0))


def test_summarize_without_the_optional_families_gives_the_base_keys_only():
    res = _result()
    base = {k: res[k] for k in ("whole", "track", "active", "plan")}
    s = SC.summarize(base)
    assert list(s) == KEYS[:5]
    full = SC.summarize(res)
    assert all(_same(s[k], full[k]) for k in KEYS[1:5]) and s["metrics"] == full["metrics"]
