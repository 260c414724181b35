"""CPU: the binaural target of m2h.separate -- the argument checks of m2h_sep_bin_rows (a negative status and a message before any
launch) and the CPU reference (tests/separate_binaural_ref.py) against the direct composition.  No GPU needed.  The argument errors
of Separator.separate(output=...) are in tests/test_gpu_separate_binaural.py: the constructor needs a GPU device."""
import numpy as np
import torch

import m2h_oracle as O
import separate_binaural_ref as BREF
import separate_ref as REF
from m2h import _lib, synthetic


def test_sep_bin_rows_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    p = 4096   # any non-null, 16-byte aligned value: never dereferenced on a rejected call
    cases = [
        ((None, p, p, 1, None), b"sep_bin_rows: null"),
        ((p, None, p, 1, None), b"sep_bin_rows: null"),
        ((p, p, None, 1, None), b"sep_bin_rows: null"),
        ((p, p, p, 0, None), b"sep_bin_rows: bad sizes"),
        ((p, p, p, -2, None), b"sep_bin_rows: bad sizes"),
        ((p, p, p, (1 << 20) + 1, None), b"sep_bin_rows: bad sizes"),
        ((p, p + 4, p, 1, None), b"sep_bin_rows: buffers"),          # misaligned masks
        ((p + 8, p, p + 8, 1, None), b"sep_bin_rows: buffers"),      # in place, misaligned
    ]
    for args, msg in cases:
        assert lib.m2h_sep_bin_rows(*args) < 0, args
        assert msg in lib.m2h_last_error(), (args, lib.m2h_last_error())
    assert lib.m2h_launch_count() == n0


def test_reference_of_one_second_is_the_direct_composition():
    """For L = 16000 the helper is np_stft -> get_binSepMasks -> np_istft((max(m, 0) * X) as complex64), called directly."""
    sd = REF.torch_state_dict(synthetic.make_state_dict(synthetic.passive_shapes(), 3))
    wave = REF.tone_noise(1, 16000, 11)
    y, masks = BREF.separate(sd, wave, 4)
    assert y.shape == (1, 2, 16000) and masks.shape == (1, 1, 512, 32, 2)
    mag, _ = O.np_stft_features(wave)
    with torch.no_grad():
        m = O.get_binSepMasks(sd, torch.from_numpy(mag), torch.tensor([[4]])).numpy()
    assert np.array_equal(masks[0, 0], m[0])
    assert (m < 0).mean() > 0.1 and (m > 0).mean() > 0.1            # the clamp is live on these weights
    for c in range(2):
        X = O.np_stft(wave[0, c])
        want = O.np_istft((np.maximum(m[0, :, :, c], 0) * X).astype(np.complex64), 512, 16000)
        assert np.array_equal(y[0, c], want)
    assert np.isfinite(y).all() and np.abs(y[0, 0]).max() > 0 and np.abs(y[0, 1]).max() > 0
    assert not np.array_equal(y[0, 0], y[0, 1])
