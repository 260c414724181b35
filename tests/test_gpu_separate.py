"""GPU: m2h.separate (long binaural recordings in, target waveforms out) against its CPU reference (tests/separate_ref.py).

Weights: synthetic.make_state_dict(synthetic.policy_shapes(), seed).  Inputs: noise (sigma 0.05) plus a tone, as
tests/test_gpu_stft.py -- the noise floor is a condition of the comparisons: it keeps every bin of every non-empty frame away from
zero, so the downmix phasor is well conditioned, while the empty frames of a cut last segment are exactly zero and exercise the
guard.  No bin is excluded from any comparison.

Bounds: the transform kernels carry the bounds of tests/test_gpu_stft.py (2e-5 magnitudes, 5e-5 complex values and waveforms); the
end-to-end waveform and P carry the project's parity contract, rel-L1 <= 1e-3 -- the pipeline amplifies a relative
error of its STFT about 2.5x, linearly (1e-5 -> 2.4e-5 on the CPU reference); chunking may change the U-Net engines with the batch
size, so P carries the fp32 U-Net bound of tests/test_gpu_unet.py (2e-5).  Memory-on cases stay at <= 4 segments: the synthetic
memory weights are not contractive and expm1 would overflow on long runs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import separate_ref as REF
from m2h import ops, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def policy_sd():
    return synthetic.make_state_dict(synthetic.policy_shapes(), SEED)


@pytest.fixture(scope="module")
def transforms(dev):
    from m2h.audio.stft import ISTFT, STFT
    fwd, inv = STFT(dev), ISTFT(dev)
    win = torch.cat((fwd.window, torch.zeros(1, device=dev)))
    return fwd.W, win, inv.W, inv.window


def test_frames_and_post_match_np_stft_per_segment(dev, transforms):
    Wf, win, _, _ = transforms
    R, L = 2, 40000
    wave = REF.tone_noise(R, L, 21)
    X = REF.segment_stft(wave)                       # [S, R, 2, 512, 32]
    S = X.shape[0]
    w = torch.from_numpy(wave).to(dev)
    parts = []
    for s0, ns in ((0, 2), (2, 1)):                  # two calls: the segment offset is exercised too
        frames = ops.sep_frames(w, win, s0, ns)
        spec = ops.linear(frames, Wf, None, name="test.dft")
        parts.append(ops.sep_stft_post(spec, ns * R))
    mag = torch.cat([p[0] for p in parts]).cpu().numpy().reshape(S, R, 512, 32, 2)
    ph = torch.cat([p[1] for p in parts]).cpu().numpy().reshape(S, R, 512, 32, 2)
    e_mag = REF.rel_l1(mag, REF.features_of(X))
    phc = ph[..., 0] + 1j * ph[..., 1]
    D = X[:, :, 0] + X[:, :, 1]
    zero = D == 0
    want = np.abs(X[:, :, 0]).astype(np.float64) * REF.phasor_of(X)
    got = np.expm1(mag[..., 0].astype(np.float64)) * phc
    e_z = REF.rel_l1(got, want)
    print("frames+post: rel-L1 magnitudes %.3e, |X_left| * phasor %.3e, exactly-zero downmix bins %.1f %% (last segment %.1f %%)"
          % (e_mag, e_z, 100 * zero.mean(), 100 * zero[-1].mean()))
    assert e_mag < 2e-5
    assert e_z < 5e-5
    assert zero[-1].mean() > 0.3 and np.all(ph[zero] == np.array([1.0, 0.0], np.float32))      # the exact-zero guard
    assert np.abs(np.abs(phc) - 1.0).max() < 1e-6


@pytest.mark.parametrize("L", [40000, 32000, 16001])
def test_inverse_pre_and_overlap_add_match_np_istft(dev, transforms, L):
    _, _, Wi, win = transforms
    R = 3
    S = -(-L // 16000)
    rng = np.random.default_rng(31)
    P = (rng.standard_normal((S, R, 512, 32)) * 1.5).astype(np.float32)          # negative values: the max(P, 0) clamp
    ang = rng.uniform(-np.pi, np.pi, (S, R, 512, 32))
    ph = np.exp(1j * ang)
    ph[rng.random(ph.shape) < 0.1] = 1.0                                        # guarded bins
    want = REF.inverse(P, ph.astype(np.complex64).astype(np.complex128), L)
    ph32 = np.stack((ph.real, ph.imag), -1).astype(np.float32)
    y = torch.full((R, L), float("nan"), device=dev)
    for s0, ns in ((0, 1), (1, S - 1)) if S > 1 else ((0, 1),):
        rows = ops.sep_istft_pre(torch.from_numpy(P[s0:s0 + ns].reshape(ns * R, 512, 32, 1)).to(dev),
                                 torch.from_numpy(ph32[s0:s0 + ns].reshape(ns * R, 512, 32, 2)).to(dev))
        frames = ops.linear(rows, Wi, None, name="test.idft")
        ops.sep_istft_ola(frames, win, y, s0, ns)
    y = y.cpu().numpy()
    e = REF.rel_l1(y, want)
    print("pre+ola L=%d: rel-L1 %.3e" % (L, e))
    assert np.isfinite(y).all()
    assert e < 5e-5


def _separator(sd, dev, math, **kw):
    from m2h.separate import Separator
    return Separator(sd, dev, math=math, **kw)


@pytest.mark.parametrize("math", [ops.MATH_FP32, ops.MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("use_memory", [True, False], ids=["memory", "nomemory"])
def test_end_to_end_matches_reference(dev, policy_sd, math, use_memory):
    R, L = 2, 40000
    wave = REF.tone_noise(R, L, 41)
    tc = [4, 7]
    want_y, want_P, want_ph = REF.separate(REF.torch_state_dict(policy_sd), wave, tc, use_memory)
    sep = _separator(policy_sd, dev, math)
    y, P, ph = sep.separate(torch.from_numpy(wave).to(dev), tc, use_memory=use_memory, return_spectrograms=True)
    assert y.shape == (R, L) and P.shape == (R, 3, 512, 32) and ph.shape == (R, 3, 512, 32, 2)
    assert ops.math_mode() == ops.MATH_FP32            # the separator's arithmetic does not leak into the calling thread
    e_y, e_P = REF.rel_l1(y.cpu().numpy(), want_y), REF.rel_l1(P.cpu().numpy(), want_P)
    print("end to end [%s, memory %s]: rel-L1 waveform %.3e, P %.3e, max|P| %.2f"
          % ("fp32" if math == ops.MATH_FP32 else "bf16x3", "on" if use_memory else "off", e_y, e_P, float(P.abs().max())))
    assert torch.isfinite(y).all()
    assert e_y <= 1e-3 and e_P <= 1e-3
    if use_memory and math == ops.MATH_FP32:
        # the default is the checkpoint's own: it has a memory
        y2 = sep.separate(torch.from_numpy(wave).to(dev), tc)
        assert torch.equal(y2, y)


def test_target_class_changes_the_output(dev, policy_sd):
    wave = torch.from_numpy(REF.tone_noise(1, 24000, 42)).to(dev)
    sep = _separator(policy_sd, dev, ops.MATH_FP32)
    a = sep.separate(wave, 4, use_memory=False).cpu().numpy()
    b = sep.separate(wave[0], 7, use_memory=False).cpu().numpy()       # the [2, L] form
    assert a.shape == (1, 24000) and b.shape == (24000,)
    change = REF.rel_l1(b, a[0])
    print("target class 4 -> 7: rel change %.3f" % change)
    assert change > 0.1
    # one class per recording is the same as each recording on its own, up to the engines the U-Nets pick for another batch size:
    # their fp32 bound on P (2e-5) times the pipeline's 2.5x amplification, plus the inverse transform's own bound (5e-5)
    both = sep.separate(torch.cat((wave, wave)), [4, 7], use_memory=False).cpu().numpy()
    assert REF.rel_l1(both[0], a[0]) < 1e-4 and REF.rel_l1(both[1], b) < 1e-4


def test_chunking_does_not_change_the_result(dev, policy_sd):
    R = 2
    wave = torch.from_numpy(REF.tone_noise(R, 160000, 43)).to(dev)
    tc = [4, 7]
    ya, Pa, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=2).separate(wave, tc, use_memory=False, return_spectrograms=True)
    yb, Pb, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=64).separate(wave, tc, use_memory=False, return_spectrograms=True)
    e = REF.rel_l1(Pa.cpu().numpy(), Pb.cpu().numpy())
    print("chunks of 1 segment x 2 recordings against one chunk, 10 s, memory off: rel-L1 P %.3e waveform %.3e"
          % (e, REF.rel_l1(ya.cpu().numpy(), yb.cpu().numpy())))
    assert Pa.shape == (R, 10, 512, 32) and e < 2e-5
    # the memory's recurrence runs across chunk borders: 4 segments as 2 + 2 against unchunked
    wave4 = wave[:, :, :64000].contiguous()
    yc, Pc, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=2 * R).separate(wave4, tc, use_memory=True, return_spectrograms=True)
    yd, Pd, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=64).separate(wave4, tc, use_memory=True, return_spectrograms=True)
    e = REF.rel_l1(Pc.cpu().numpy(), Pd.cpu().numpy())
    print("memory on, 4 segments as 2 + 2 against unchunked: rel-L1 P %.3e" % e)
    assert torch.isfinite(yc).all() and e < 2e-5
    assert REF.rel_l1(Pd[:, 3].cpu().numpy(), Pb[:, 3].cpu().numpy()) > 1e-2    # and the memory does something


def test_checkpoint_forms_and_argument_errors(dev, policy_sd, tmp_path):
    passive = {k: v for k, v in policy_sd.items() if k.startswith(("binSep_", "bin2mono_"))}
    assert len(passive) == 124
    wave = torch.from_numpy(REF.tone_noise(1, 20000, 44)).to(dev)
    plain = _separator(passive, dev, ops.MATH_FP32)
    assert plain.memory is None
    y0 = plain.separate(wave, 3)                      # default: no memory, the checkpoint has none
    with pytest.raises(RuntimeError, match="no acoustic_mem"):
        plain.separate(wave, 3, use_memory=True)
    # a PPO checkpoint file in the trainer's format gives the same separators (memory off) and has a memory
    path = str(tmp_path / "ckpt.pth")
    torch.save({"state_dict": {"actor_critic." + k: torch.from_numpy(np.asarray(v)) for k, v in policy_sd.items()}, "config": {}}, path)
    full = _separator(path, dev, ops.MATH_FP32)
    assert full.memory is not None
    assert torch.equal(full.separate(wave, 3, use_memory=False), y0)
    assert not torch.equal(full.separate(wave, 3), y0)
    with pytest.raises(RuntimeError, match="cpu"):
        full.separate(wave.cpu(), 3)
    with pytest.raises(RuntimeError, match=r"\(1, 1, 20000\)"):
        full.separate(wave[:, :1].contiguous(), 3)
    with pytest.raises(RuntimeError, match="float64"):
        full.separate(wave.double(), 3)
    with pytest.raises(RuntimeError, match="target_class"):
        full.separate(wave, [1, 2, 3])


@pytest.mark.parametrize("fmt", ["int16", "float32"])
def test_cli_round_trip(dev, policy_sd, tmp_path, fmt):
    from scipy.io import wavfile
    L = 36000
    wave = REF.tone_noise(1, L, 45)[0]                 # [2, L]
    if fmt == "int16":
        samples = np.clip(np.rint(wave.T * 32768.0), -32768, 32767).astype(np.int16)
        as_float = samples.astype(np.float32).T * np.float32(1.0 / 32768.0)
    else:
        samples = np.ascontiguousarray(wave.T)
        as_float = wave
    inp, out, ckpt = str(tmp_path / "mix.wav"), str(tmp_path / "out.wav"), str(tmp_path / "ckpt.pth")
    wavfile.write(inp, 16000, samples)
    torch.save({"state_dict": {"actor_critic." + k: torch.from_numpy(np.asarray(v)) for k, v in policy_sd.items()}, "config": {}}, ckpt)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "separate.py"), "--ckpt", ckpt, "--in", inp, "--target-class", "5", "--out", out,
                        "--math", "fp32"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    rate, got = wavfile.read(out)
    assert rate == 16000 and got.shape == (L,) and got.dtype == samples.dtype
    y = _separator(policy_sd, dev, ops.MATH_FP32).separate(torch.from_numpy(np.ascontiguousarray(as_float)).to(dev), 5).cpu().numpy()
    if fmt == "int16":
        want = np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    else:
        want = y
    assert np.array_equal(got, want)
    # a wrong sample rate is an error, not a resampling
    wavfile.write(inp, 8000, samples)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "separate.py"), "--ckpt", ckpt, "--in", inp, "--target-class", "5", "--out", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode != 0 and "16000" in r.stdout
