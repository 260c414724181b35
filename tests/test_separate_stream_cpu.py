"""CPU: the pure-Python statements of a streamed separation (m2h.separate.stream_emitted / stream_returned,
m2h.audio.resample.ready_outputs) and the argument checks of the window entry points (a negative status and a message before any
launch).  No GPU needed."""
import numpy as np
import pytest

from m2h import _lib
from m2h.audio.resample import ratio, ready_outputs
from m2h.separate import stream_emitted, stream_returned

RATES = (8000, 11025, 22050, 44100, 48000, 96000)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_stream_emitted_at_the_edges(k):
    H = 16000 // k
    assert stream_emitted(0, k) == 0
    assert stream_emitted(15999, k) == 0
    assert stream_emitted(16000, k) == H                 # segment 0 is done: the samples no later segment covers
    assert stream_emitted(16001, k) == H
    assert stream_emitted(16000 + H - 1, k) == H
    assert stream_emitted(16000 + H, k) == 2 * H
    P = np.arange(0, 70000, dtype=np.int64)
    E = stream_emitted(P, k)
    assert E.tolist() == [stream_emitted(int(p), k) for p in P]
    # the statement itself: segment s is processed once sample s*H + 15999 is there; a sample is final below the next segment's start
    done = np.where(P >= 16000, (P - 16000) // H + 1, 0)
    assert np.array_equal(E, done * H) and np.all(E <= P)
    for bad in (0, 3, True, None):
        with pytest.raises(ValueError):
            stream_emitted(16000, bad)


@pytest.mark.parametrize("f_in,f_out", [(44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000), (1023, 1000), (8000, 16000), (16000, 8000)])
def test_converter_readiness_is_the_brute_force_count(f_in, f_out):
    up, down = ratio(f_in, f_out)
    half = 10 * max(up, down)
    for P in list(range(0, 60)) + [97, 441, 499, 1500, 2001, 5003]:
        n, count = 0, 0
        while (n * down + half) // up < P:               # output n is emitted once input sample (n*down + half) div up has arrived
            n, count = n + 1, count + 1
        assert ready_outputs(P, up, down) == count, (P, up, down)
        assert count <= -(-P * up // down)
    P = np.arange(0, 3000, dtype=np.int64)
    assert ready_outputs(P, up, down).tolist() == [ready_outputs(int(p), up, down) for p in P]


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("f", RATES)
def test_backlog_stays_under_1_01_seconds(f, k):
    P = np.arange(0, 3 * f + 1, dtype=np.int64)
    E = stream_returned(P, f, k)
    backlog = P - E
    print("%d Hz overlap %d: worst backlog %.4f s at P = %d" % (f, k, backlog.max() / f, int(P[backlog.argmax()])))
    assert np.all(E >= 0) and np.all(np.diff(E) >= 0) and np.all(backlog >= 0)
    assert backlog.max() <= 1.01 * f
    assert E[-1] > 0
    assert stream_returned(int(P[-1]), f, k) == E[-1]
    assert np.array_equal(stream_returned(P[:40000], 16000, k), stream_emitted(P[:40000], k))


def test_window_entry_points_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    p = 4096   # any non-null, 16-byte aligned value: never dereferenced on a rejected call
    cases = [
        # buf, window, frames, R, cap, origin, end, hop, s0, nseg
        ("m2h_sep_frames_win", (None, p, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_frames_win: null"),
        ("m2h_sep_frames_win", (p, None, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_frames_win: null"),
        ("m2h_sep_frames_win", (p, p, None, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_frames_win: null"),
        ("m2h_sep_frames_win", (p, p, p, 1, 16000, 0, 16000, 5000, 0, 1, None), b"sep_frames_win: hop"),
        ("m2h_sep_frames_win", (p, p, p, 1, 16000, 0, 16000, 0, 0, 1, None), b"sep_frames_win: hop"),
        ("m2h_sep_frames_win", (p, p, p, 0, 16000, 0, 16000, 8000, 0, 1, None), b"sep_frames_win: bad sizes"),
        ("m2h_sep_frames_win", (p, p, p, 1, 0, 0, 16000, 8000, 0, 1, None), b"sep_frames_win: bad sizes"),
        ("m2h_sep_frames_win", (p, p, p, 1, 16000, -4, 16000, 8000, 0, 1, None), b"sep_frames_win: bad sizes"),
        ("m2h_sep_frames_win", (p, p, p, 1, 16000, 0, 16000, 8000, 0, 0, None), b"sep_frames_win: bad sizes"),
        ("m2h_sep_frames_win", (p, p, p, 1, 16000, 0, 16000, 8000, 2, 1, None), b"sep_frames_win: bad sizes"),        # segment 2 of 2
        ("m2h_sep_frames_win", (p, p, p, 1, 15999, 0, 16000, 8000, 0, 1, None), b"leave the window"),                 # one sample short
        ("m2h_sep_frames_win", (p, p, p, 1, 20000, 8004, 24001, 4000, 2, 1, None), b"leave the window"),              # starts before the origin
        ("m2h_sep_frames_win", (p, p, p, 1, 16000, 8000, 24001, 4000, 2, 2, None), b"leave the window"),              # [8000, 24001) in 16000
        ("m2h_sep_frames_win", (p, p + 4, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_frames_win: window"),
        # frames, window, y, R, cap, origin, end, s0, nseg
        ("m2h_sep_istft_ola_win", (None, p, p, 1, 16000, 0, 16000, 0, 1, None), b"sep_istft_ola_win: null"),
        ("m2h_sep_istft_ola_win", (p, None, p, 1, 16000, 0, 16000, 0, 1, None), b"sep_istft_ola_win: null"),
        ("m2h_sep_istft_ola_win", (p, p, None, 1, 16000, 0, 16000, 0, 1, None), b"sep_istft_ola_win: null"),
        ("m2h_sep_istft_ola_win", (p, p, p, 1, 16000, 0, 16000, 0, 0, None), b"sep_istft_ola_win: bad sizes"),
        ("m2h_sep_istft_ola_win", (p, p, p, 1, 16000, 0, 16000, 1, 1, None), b"sep_istft_ola_win: bad sizes"),        # segment 1 of 1
        ("m2h_sep_istft_ola_win", (p, p, p, 1, 16000, 0, 16001, 0, 2, None), b"leave the window"),                    # [0, 16001) in 16000
        ("m2h_sep_istft_ola_win", (p, p, p, 1, 16000, 16000, 32000, 0, 1, None), b"leave the window"),                # before the origin
        # frames, window, xwin, y, R, cap, origin, end, hop, s0, nseg
        ("m2h_sep_istft_xfade_win", (None, p, p, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_istft_xfade_win: null"),
        ("m2h_sep_istft_xfade_win", (p, None, p, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_istft_xfade_win: null"),
        ("m2h_sep_istft_xfade_win", (p, p, None, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_istft_xfade_win: null"),
        ("m2h_sep_istft_xfade_win", (p, p, p, None, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_istft_xfade_win: null"),
        ("m2h_sep_istft_xfade_win", (p, p, p, p, 1, 16000, 0, 16000, 5000, 0, 1, None), b"sep_istft_xfade_win: hop"),
        ("m2h_sep_istft_xfade_win", (p, p, p, p, 1, 16000, 0, 16000, 8000, 0, 0, None), b"sep_istft_xfade_win: bad sizes"),
        ("m2h_sep_istft_xfade_win", (p, p, p, p, 1, 16000, 0, 16000, 8000, 0, 3, None), b"sep_istft_xfade_win: bad sizes"),   # [0, 3) of 2
        ("m2h_sep_istft_xfade_win", (p, p, p, p, 1, 16000, 4000, 24001, 4000, 1, 2, None), b"leave the window"),             # [4000, 24000) in 16000
        ("m2h_sep_istft_xfade_win", (p, p, p, p, 1, 16000, 8000, 24001, 4000, 1, 1, None), b"leave the window"),
        ("m2h_sep_istft_xfade_win", (p, p, p + 4, p, 1, 16000, 0, 16000, 8000, 0, 1, None), b"sep_istft_xfade_win: the cross-fade window"),
        # x, G, y, rows, cap, origin, end, n_first, count, up, down, T   (3 -> 1: half 30, T 61, outputs < ceil(end / 3))
        ("m2h_resample_poly_win", (None, p, p, 1, 3000, 0, 3000, 0, 100, 1, 3, 61, None), b"resample_poly_win: null"),
        ("m2h_resample_poly_win", (p, None, p, 1, 3000, 0, 3000, 0, 100, 1, 3, 61, None), b"resample_poly_win: null"),
        ("m2h_resample_poly_win", (p, p, None, 1, 3000, 0, 3000, 0, 100, 1, 3, 61, None), b"resample_poly_win: null"),
        ("m2h_resample_poly_win", (p, p, p, 0, 3000, 0, 3000, 0, 100, 1, 3, 61, None), b"resample_poly_win: bad sizes"),
        ("m2h_resample_poly_win", (p, p, p, 1, 0, 0, 3000, 0, 100, 1, 3, 61, None), b"resample_poly_win: bad sizes"),
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 0, 3000, -1, 100, 1, 3, 61, None), b"resample_poly_win: bad sizes"),
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 0, 3000, 0, 0, 1, 3, 61, None), b"resample_poly_win: count"),
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 0, 3000, 0, -5, 1, 3, 61, None), b"resample_poly_win: count"),
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 0, 3000, 0, 1001, 1, 3, 61, None), b"pass ceil"),                       # ceil(3000 / 3) = 1000
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 0, 3000, 0, 100, 1, 3, 60, None), b"resample_poly_win: a table of T 60"),
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 0, 3000, 0, 100, 1, 1025, 20501, None), b"over the limit"),
        ("m2h_resample_poly_win", (p + 2, p, p, 1, 3000, 0, 3000, 0, 100, 1, 3, 61, None), b"resample_poly_win: buffers"),
        # output 100 reads x[(300 + 30) - 60 .. 330] = [270, 331): a window from 271 on, or one that ends at 330, does not hold them
        ("m2h_resample_poly_win", (p, p, p, 1, 3000, 271, 3000, 100, 1, 1, 3, 61, None), b"outside the window"),
        ("m2h_resample_poly_win", (p, p, p, 1, 60, 270, 3000, 100, 1, 1, 3, 61, None), b"outside the window"),
    ]
    for name, args, msg in cases:
        assert getattr(lib, name)(*args) < 0, (name, args)
        assert msg in lib.m2h_last_error(), (name, args, lib.m2h_last_error())
    assert lib.m2h_launch_count() == n0


def test_stream_checks_its_arguments_like_separate():
    from m2h.separate import Separator, SeparatorStream
    sep = Separator.__new__(Separator)                                   # no device needed to reach the checks
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    for bad in (0, 3, 8, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="overlap"):
            sep.stream(4, recordings=1, overlap=bad)
    with pytest.raises(ValueError, match="output"):
        sep.stream(4, recordings=1, output="stereo")
    with pytest.raises(ValueError, match="binaural"):
        sep.stream(4, recordings=1, output="binaural", use_memory=True)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="recordings"):
            sep.stream(4, recordings=bad)
    with pytest.raises(TypeError):
        sep.stream(4, recordings=1, return_spectrograms=True)            # not offered on a stream
    assert SeparatorStream.push is not None and lib.m2h_launch_count() == n0
