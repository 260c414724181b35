"""CPU: the rate conversion's definition (m2h/audio/resample.py) against scipy, its lengths and limits, and the argument checks of
m2h_resample_poly (a negative status and a message before any launch).  No GPU needed."""
import numpy as np
import pytest

import resample_ref as RR
from m2h import _lib
from m2h.audio import resample as RS


@pytest.mark.parametrize("f_in,f_out", RR.RATES)
def test_design_is_scipy_firwin_times_up(f_in, f_out):
    from scipy.signal import firwin
    up, down, half, h = RS.design(f_in, f_out)
    assert (up, down) == RR.ratio(f_in, f_out) and half == 10 * max(up, down) and h.dtype == np.float64 and h.shape == (2 * half + 1,)
    want = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert np.abs(h - want).max() < 1e-12
    assert np.array_equal(h, RR.taps(f_in, f_out)[3])
    assert RS.taps_per_output(up, down) == RR.TAPS[(f_in, f_out)]
    G = RS.polyphase_table(h, up)
    T = RR.TAPS[(f_in, f_out)]
    assert G.shape == (up, T) and G.flags["C_CONTIGUOUS"]
    flat = G.T.reshape(-1)                              # [k][p] order is h followed by zeros
    assert np.array_equal(flat[:len(h)], h) and not flat[len(h):].any()


@pytest.mark.parametrize("f_in,f_out", RR.RATES)
@pytest.mark.parametrize("L", [1, 5, 1023, 3000])
def test_restatement_is_scipy_resample_poly(f_in, f_out, L):
    up, down, half, h = RR.taps(f_in, f_out)
    x = RR.tone_noise(3, L, 7, f_in).astype(np.float64)
    want = RR.scipy_resample(x, up, down)
    a, b = RR.direct(x, h, up, down, half), RR.polyphase(x, h, up, down, half)
    assert want.shape == a.shape == b.shape == (3, RR.out_len(L, up, down))
    assert np.abs(a - want).max() < 1e-12 and np.abs(b - want).max() < 1e-12
    lo = min(7, b.shape[1] - 1)
    assert np.array_equal(RR.polyphase(x, h, up, down, half, lo, b.shape[1]), b[:, lo:])       # a window of outputs is the same sum


def test_lengths_limit_and_identity():
    assert RS.ratio(48000, 16000) == (1, 3) and RS.ratio(44100, 16000) == (160, 441) and RS.ratio(16000, 44100) == (441, 160)
    assert RS.output_length(70003, 160, 441) == 25398 and RS.output_length(1, 1, 3) == 1 and RS.output_length(3, 1, 3) == 1
    assert RS.output_length(4, 1, 3) == 2 and RS.output_length(5, 441, 160) == 14
    assert RS.ratio(1024, 1) == (1, 1024) and RS.ratio(16000, 16384) == (128, 125)
    with pytest.raises(ValueError, match="16001/16000"):
        RS.design(16000, 16001)
    with pytest.raises(ValueError, match="1/1025"):
        RS.ratio(1025, 1)
    for bad in ((0, 16000), (16000, -1), (44100.5, 16000)):
        with pytest.raises(ValueError):
            RS.ratio(*bad)
    # the identity needs neither a GPU nor a launch
    import torch
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    r = RS.Resampler(16000, 16000, torch.device("cpu"))
    x = torch.zeros(2, 5)
    assert r.identity and r.table is None and r(x) is x and (r.up, r.down) == (1, 1)
    assert lib.m2h_launch_count() == n0
    with pytest.raises(RuntimeError, match="GPU"):
        RS.Resampler(44100, 16000, torch.device("cpu"))


def test_back_conversion_is_never_short():
    for f in (44100, 48000, 22050, 8000, 11025, 32000, 96000):
        a, b = RS.ratio(f, 16000)
        for L in list(range(1, 2000)) + [70003, 13500000, 2 ** 31 + 11]:
            L16 = RS.output_length(L, a, b)
            assert RS.output_length(L16, b, a) >= L, (f, L)


def test_entry_point_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    p = 4096   # any non-null aligned value: never dereferenced on a rejected call
    cases = [
        ((None, p, p, 1, 3000, 1000, 1, 3, 61, None), b"resample_poly: null"),
        ((p, None, p, 1, 3000, 1000, 1, 3, 61, None), b"resample_poly: null"),
        ((p, p, None, 1, 3000, 1000, 1, 3, 61, None), b"resample_poly: null"),
        ((p, p, p, 0, 3000, 1000, 1, 3, 61, None), b"resample_poly: bad sizes"),
        ((p, p, p, 1, 0, 0, 1, 3, 61, None), b"resample_poly: bad sizes"),
        ((p, p, p, 1, 3000, 1000, 0, 3, 61, None), b"resample_poly: bad sizes"),
        ((p, p, p, 1, 3000, 1000, 1, 3, 0, None), b"resample_poly: bad sizes"),
        ((p, p, p, 1, 3001, 1000, 1, 3, 61, None), b"resample_poly: L_out 1000 is not ceil"),     # ceil(3001 / 3) = 1001
        ((p, p, p, 1, 3000, 1001, 1, 3, 61, None), b"resample_poly: L_out 1001 is not ceil"),
        ((p, p, p, 1, 3000, 1000, 1, 3, 60, None), b"resample_poly: a table of T 60"),            # 60 < 2 * 30 + 1
        ((p, p, p, 1, 441, 160, 160, 441, 55, None), b"resample_poly: a table of T 55"),          # 55 * 160 < 8821
        ((p, p, p, 1, 1025, 1, 1, 1025, 20501, None), b"resample_poly: ratio 1/1025 is over the limit"),
        ((p, p, p, 1, 1, 1025, 1025, 1, 21, None), b"resample_poly: ratio 1025/1 is over the limit"),
        ((p + 2, p, p, 1, 3000, 1000, 1, 3, 61, None), b"resample_poly: buffers"),
    ]
    for args, msg in cases:
        assert lib.m2h_resample_poly(*args) < 0, args
        assert msg in lib.m2h_last_error(), (args, lib.m2h_last_error())
    assert lib.m2h_launch_count() == n0
