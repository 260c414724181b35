"""CPU: the separation path's chunk plan, its CPU reference, the argument checks of its four C entry points (a negative status and a
message before any launch) and the checkpoint-form detection.  No GPU needed."""
import numpy as np
import pytest
import torch

import m2h_oracle as O
import separate_ref as REF
from m2h import _lib, synthetic


def test_segment_plan_edges():
    from m2h.separate import segment_plan
    assert segment_plan(1, 64) == [(0, 1)]
    assert segment_plan(16000, 64) == [(0, 1)]
    assert segment_plan(16001, 64) == [(0, 2)]
    assert segment_plan(16001, 1) == [(0, 1), (1, 1)]
    assert segment_plan(10 * 16000, 2) == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 2)]          # splits evenly
    assert segment_plan(10 * 16000, 4) == [(0, 4), (4, 4), (8, 2)]                          # does not
    assert segment_plan(10 * 16000 - 1, 10) == [(0, 10)]
    plan = segment_plan(3600 * 16000 + 5, 64)
    assert sum(n for _, n in plan) == 3601 and all(0 < n <= 64 for _, n in plan)
    assert [s for s, _ in plan] == [sum(n for _, n in plan[:i]) for i in range(len(plan))]
    for bad in ((0, 4), (-3, 4), (16000, 0)):
        with pytest.raises(ValueError):
            segment_plan(*bad)


def test_reference_of_one_second_is_the_direct_composition():
    """For L = 16000 the helper is np_stft_features -> pair -> np_istft called directly (with the downmix phase)."""
    sd = REF.torch_state_dict(synthetic.make_state_dict(synthetic.passive_shapes(), 3))
    wave = REF.tone_noise(1, 16000, 11)
    y, P, ph = REF.separate(sd, wave, 4, use_memory=False)
    mag, _ = O.np_stft_features(wave)
    with torch.no_grad():
        _, mono = O.passive_pair(sd, torch.from_numpy(mag), torch.tensor([[4]]))
    D = O.np_stft(wave[0, 0]).astype(np.complex128) + O.np_stft(wave[0, 1]).astype(np.complex128)
    Z = (np.expm1(np.maximum(mono[0, :, :, 0].numpy().astype(np.float64), 0.0)) * np.exp(1j * np.angle(D))).astype(np.complex64)
    want = O.np_istft(Z, 512, 16000)
    assert y.shape == (1, 16000) and P.shape == (1, 1, 512, 32) and ph.shape == (1, 1, 512, 32)
    assert np.array_equal(P[0, 0], mono[0, :, :, 0].numpy())
    assert np.array_equal(y[0], want) and np.isfinite(y).all() and np.abs(y).max() > 0


def test_reference_pads_cuts_and_guards_zero_bins():
    wave = REF.tone_noise(2, 40000, 12)
    X = REF.segment_stft(wave)
    assert X.shape == (3, 2, 2, 512, 32)
    ph = REF.phasor_of(X)
    D = X[:, :, 0] + X[:, :, 1]
    assert np.all(ph[D == 0] == 1.0) and (D[2] == 0).mean() > 0.3 and not (D[:2] == 0).any()   # empty frames of the last segment
    assert np.allclose(np.abs(ph), 1.0)
    P = np.log1p(np.abs(X[:, :, 0])).astype(np.float32)
    y = REF.inverse(P, ph, 40000)
    assert y.shape == (2, 40000)
    assert np.array_equal(REF.segments(wave)[2, :, :, 8000:], np.zeros((2, 2, 8000), np.float32))


def test_entry_points_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    p = 4096   # any non-null, 16-byte aligned value: never dereferenced on a rejected call
    cases = [
        ("m2h_sep_frames", (None, p, p, 1, 16000, 0, 1, None), b"sep_frames: null"),
        ("m2h_sep_frames", (p, p, p, 0, 16000, 0, 1, None), b"sep_frames: bad sizes"),
        ("m2h_sep_frames", (p, p, p, 1, 0, 0, 1, None), b"sep_frames: bad sizes"),
        ("m2h_sep_frames", (p, p, p, 1, 16001, 1, 2, None), b"sep_frames: bad sizes"),          # segments [1, 3) of 2
        ("m2h_sep_frames", (p, p, p, 1, (1 << 40) + 1, 0, 1, None), b"sep_frames: bad sizes"),  # the window forms' limit, L <= 2^40
        ("m2h_sep_frames", (p, p + 4, p, 1, 16000, 0, 1, None), b"sep_frames: window"),
        ("m2h_sep_stft_post", (p, None, p, 1, None), b"sep_stft_post: null"),
        ("m2h_sep_stft_post", (p, p, p, 0, None), b"sep_stft_post: bad sizes"),
        ("m2h_sep_stft_post", (p, p, p + 8, 1, None), b"sep_stft_post: buffers"),
        ("m2h_sep_istft_pre", (p, p, None, 1, None), b"sep_istft_pre: null"),
        ("m2h_sep_istft_pre", (p, p, p, -2, None), b"sep_istft_pre: bad sizes"),
        ("m2h_sep_istft_ola", (p, None, p, 1, 16000, 0, 1, None), b"sep_istft_ola: null"),
        ("m2h_sep_istft_ola", (p, p, p, 1, 16000, 0, 2, None), b"sep_istft_ola: bad sizes"),
        ("m2h_sep_istft_ola", (p, p, p, 1, 16000, -1, 1, None), b"sep_istft_ola: bad sizes"),
        ("m2h_sep_istft_ola", (p, p, p, 1, (1 << 40) + 1, 0, 1, None), b"sep_istft_ola: bad sizes"),
    ]
    for name, args, msg in cases:
        assert getattr(lib, name)(*args) < 0, (name, args)
        assert msg in lib.m2h_last_error(), (name, args, lib.m2h_last_error())
    assert lib.m2h_launch_count() == n0


def test_checkpoint_forms():
    from m2h.separate import split_checkpoint
    passive = synthetic.make_state_dict(synthetic.passive_shapes(), 1)
    policy = synthetic.make_state_dict(synthetic.policy_shapes(), 1)
    assert len(passive) == 124
    sep, mem, variant = split_checkpoint(passive)
    assert list(sep) == list(passive) and mem is None and variant is None
    for form in (policy, {"actor_critic." + k: v for k, v in policy.items()},
                 {"state_dict": {"actor_critic." + k: v for k, v in policy.items()}, "config": {"x": 1}},
                 {"state_dict": dict(policy), "config": None}):
        sep, mem, variant = split_checkpoint(form)
        assert sorted(sep) == sorted(passive) and sorted(mem) == ["cnn.0.weight", "cnn.2.weight"] and variant == "ddppo"
        assert all(sep[k] is policy[k] for k in sep)
    bn = dict(passive)
    bn.update({"acoustic_mem.cnn.0.weight": 0, "acoustic_mem.cnn.1.weight": 0, "acoustic_mem.cnn.1.bias": 0,
               "acoustic_mem.cnn.1.running_mean": 0, "acoustic_mem.cnn.1.running_var": 0, "acoustic_mem.cnn.3.weight": 0})
    assert split_checkpoint({"state_dict": bn, "config": {}})[2] == "bn"
    with pytest.raises(RuntimeError, match="no separator weights"):
        split_checkpoint({"pol_net.x": 1})
    with pytest.raises(RuntimeError, match="must be a dict"):
        split_checkpoint([1, 2])


def test_separator_needs_a_gpu_device():
    from m2h.separate import Separator
    with pytest.raises(RuntimeError, match="GPU"):
        Separator(synthetic.make_state_dict(synthetic.passive_shapes(), 1), torch.device("cpu"))
