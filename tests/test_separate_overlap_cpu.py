"""CPU: overlapped, cross-faded segments of the separation path (m2h.separate, overlap = k): the chunk plan, the cross-fade window,
the CPU reference (tests/separate_overlap_ref.py) at its degenerate cases, and the argument checks of the two C entry points (a
negative status and a message before any launch).  No GPU needed."""
import numpy as np
import pytest

import separate_overlap_ref as OREF
import separate_ref as REF
from m2h import _lib, synthetic

LENGTHS = [1, 4000, 4001, 16000, 16001, 10 * 16000, 3600 * 16000 + 5]


@pytest.mark.parametrize("overlap", [1, 2, 4])
@pytest.mark.parametrize("L", LENGTHS)
def test_overlap_plan_edges(L, overlap):
    from m2h.separate import overlap_plan, segment_plan
    H = 16000 // overlap
    S = -(-L // H)
    for max_segments in (1, 2, 3, 4, 7, 64, 1024):          # 1 .. 3: smaller than the overlap
        plan = overlap_plan(L, overlap, max_segments)
        per = max(overlap, max_segments) // overlap * overlap
        assert sum(n for _, n in plan) == S
        assert [s for s, _ in plan] == [sum(n for _, n in plan[:i]) for i in range(len(plan))]        # contiguous, in order
        assert all(n == per for _, n in plan[:-1]) and 0 < plan[-1][1] <= per
        assert all(n % overlap == 0 and s % overlap == 0 for s, n in plan[:-1]) and plan[-1][0] % overlap == 0
        if overlap == 1:
            assert plan == segment_plan(L, max_segments)


def test_overlap_plan_examples_and_bad_arguments():
    from m2h.separate import overlap_plan
    assert overlap_plan(1, 4, 64) == [(0, 1)]
    assert overlap_plan(4000, 4, 64) == [(0, 1)] and overlap_plan(4001, 4, 64) == [(0, 2)]
    assert overlap_plan(16001, 2, 1) == [(0, 2), (2, 1)]                 # max_segments below the overlap: one step per chunk
    assert overlap_plan(16001, 4, 3) == [(0, 4), (4, 1)]
    assert overlap_plan(40000, 2, 5) == [(0, 4), (4, 1)]                 # rounded down to a multiple of the overlap
    assert overlap_plan(10 * 16000, 4, 16) == [(0, 16), (16, 16), (32, 8)]
    for bad in ((0, 2, 4), (-3, 2, 4), (16000, 2, 0), (16000, 3, 4), (16000, 0, 4), (16000, 8, 4)):
        with pytest.raises(ValueError):
            overlap_plan(*bad)


def test_crossfade_window():
    from m2h.separate import crossfade_window
    w = crossfade_window(np.float64)
    assert w.shape == (16000,) and w.dtype == np.float64
    assert w.min() > 0 and abs(w.min() - 9.64e-9) < 1e-11              # strictly positive: W > 0 at the recording's first sample
    assert np.array_equal(w, w[::-1]) or np.abs(w - w[::-1]).max() < 1e-15
    for k in (2, 4):
        H = 16000 // k
        total = sum(np.roll(w, c * H) for c in range(k))                # wherever k segments cover a sample
        assert np.abs(total - k / 2).max() < 1e-12
    w32 = crossfade_window()
    assert w32.dtype == np.float32 and np.array_equal(w32, w.astype(np.float32)) and w32.min() > 0
    assert np.array_equal(w32, w32[::-1])
    assert np.array_equal(OREF.window(), w32.astype(np.float64))         # the reference states the same window on its own


@pytest.fixture(scope="module")
def sd():
    return REF.torch_state_dict(synthetic.make_state_dict(synthetic.policy_shapes(), 2))


def test_reference_with_overlap_one_is_the_plain_reference(sd):
    wave = REF.tone_noise(1, 20000, 13)
    want = REF.separate(sd, wave, 4, True)
    got = OREF.separate(sd, wave, 4, True, 1)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)


def test_reference_of_a_recording_inside_one_hop(sd):
    """L = 3999 <= H at overlap 4: one segment, w / W = 1."""
    wave = REF.tone_noise(2, 3999, 14)
    want = OREF.separate(sd, wave, [4, 7], False, 1)
    got = OREF.separate(sd, wave, [4, 7], False, 4)
    assert got[1].shape == (2, 1, 512, 32)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0


def test_reference_crossfade_and_segment_order():
    """Constant chains come out as their weighted mean, a single covering segment as itself, P in segment order."""
    L, k = 24001, 4
    H = 16000 // k
    ys = [np.full((1, L - c * H), float(c + 1), np.float32) for c in OREF.chains(L, k)]
    y = OREF.crossfade(ys, L, k)
    assert np.array_equal(y[0, :H], np.ones(H, np.float32))              # only segment 0 covers the first hop
    w = OREF.window()
    n = 3 * H + 5
    want = sum(w[n - c * H] * (c + 1) for c in range(4)) / sum(w[n - c * H] for c in range(4))
    assert abs(float(y[0, n]) - want) < 1e-6
    assert OREF.n_segments(L, k) == 7
    parts = [np.full((1, len(range(c, 7, k)), 2), c, np.int64) + 10 * np.arange(len(range(c, 7, k)))[None, :, None] for c in range(4)]
    P = OREF.interleave(parts, L, k)
    assert P[0, :, 0].tolist() == [0, 1, 2, 3, 10, 11, 12]


def test_new_entry_points_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    p = 4096   # any non-null, 16-byte aligned value: never dereferenced on a rejected call
    cases = [
        ("m2h_sep_frames_hop", (None, p, p, 1, 16000, 8000, 0, 1, None), b"sep_frames_hop: null"),
        ("m2h_sep_frames_hop", (p, None, p, 1, 16000, 8000, 0, 1, None), b"sep_frames_hop: null"),
        ("m2h_sep_frames_hop", (p, p, None, 1, 16000, 8000, 0, 1, None), b"sep_frames_hop: null"),
        ("m2h_sep_frames_hop", (p, p, p, 1, 16000, 5000, 0, 1, None), b"sep_frames_hop: hop"),
        ("m2h_sep_frames_hop", (p, p, p, 1, 16000, 0, 0, 1, None), b"sep_frames_hop: hop"),
        ("m2h_sep_frames_hop", (p, p, p, 0, 16000, 8000, 0, 1, None), b"sep_frames_hop: bad sizes"),
        ("m2h_sep_frames_hop", (p, p, p, 1, 0, 8000, 0, 1, None), b"sep_frames_hop: bad sizes"),
        ("m2h_sep_frames_hop", (p, p, p, 1, 16001, 8000, 2, 2, None), b"sep_frames_hop: bad sizes"),      # segments [2, 4) of 3
        ("m2h_sep_frames_hop", (p, p, p, 1, 16000, 4000, 4, 1, None), b"sep_frames_hop: bad sizes"),      # segment 4 of 4
        ("m2h_sep_frames_hop", (p, p, p, 1, 16000, 4000, -1, 1, None), b"sep_frames_hop: bad sizes"),
        ("m2h_sep_frames_hop", (p, p, p, 1, (1 << 40) + 1, 8000, 0, 1, None), b"sep_frames_hop: bad sizes"),   # the window forms' limit, L <= 2^40
        ("m2h_sep_frames_hop", (p, p + 4, p, 1, 16000, 8000, 0, 1, None), b"sep_frames_hop: window"),
        ("m2h_sep_istft_xfade", (None, p, p, p, 1, 16000, 8000, 0, 1, None), b"sep_istft_xfade: null"),
        ("m2h_sep_istft_xfade", (p, None, p, p, 1, 16000, 8000, 0, 1, None), b"sep_istft_xfade: null"),
        ("m2h_sep_istft_xfade", (p, p, None, p, 1, 16000, 8000, 0, 1, None), b"sep_istft_xfade: null"),
        ("m2h_sep_istft_xfade", (p, p, p, None, 1, 16000, 8000, 0, 1, None), b"sep_istft_xfade: null"),
        ("m2h_sep_istft_xfade", (p, p, p, p, 1, 16000, 5000, 0, 1, None), b"sep_istft_xfade: hop"),
        ("m2h_sep_istft_xfade", (p, p, p, p, 1, 16000, 8000, 0, 3, None), b"sep_istft_xfade: bad sizes"),  # segments [0, 3) of 2
        ("m2h_sep_istft_xfade", (p, p, p, p, 1, 24001, 4000, 7, 1, None), b"sep_istft_xfade: bad sizes"),  # segment 7 of 7
        ("m2h_sep_istft_xfade", (p, p, p, p, 1, 16000, 8000, 0, 0, None), b"sep_istft_xfade: bad sizes"),
        ("m2h_sep_istft_xfade", (p, p, p, p, 1, (1 << 40) + 1, 8000, 0, 1, None), b"sep_istft_xfade: bad sizes"),
        ("m2h_sep_istft_xfade", (p, p, p + 4, p, 1, 16000, 8000, 0, 1, None), b"sep_istft_xfade: the cross-fade window"),
    ]
    for name, args, msg in cases:
        assert getattr(lib, name)(*args) < 0, (name, args)
        assert msg in lib.m2h_last_error(), (name, args, lib.m2h_last_error())
    assert lib.m2h_launch_count() == n0


def test_separator_rejects_other_overlaps_before_anything_else():
    """The overlap is checked first: a ValueError even for arguments that would fail later checks (no tensor, no launch)."""
    from m2h.separate import Separator
    sep = Separator.__new__(Separator)                                   # no device needed to reach the check
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    for bad in (0, 3, 8, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="overlap"):
            sep.separate(None, 4, overlap=bad)
    assert lib.m2h_launch_count() == n0
