"""GPU: the binaural target of m2h.separate (output="binaural" / "both") against its CPU reference (tests/separate_binaural_ref.py).

Weights and inputs as tests/test_gpu_separate.py: synthetic.make_state_dict(synthetic.policy_shapes(), 2) and noise (sigma 0.05) plus a
tone.  No bin or sample is excluded from any comparison.

Bounds: m2h_sep_bin_rows is one fp32 multiply per element and is compared bit for bit.  End to end the waveform and the masks carry the
project's parity contract, rel-L1 <= 1e-3: after the clamp the map from masks to waveform is linear, so nothing amplifies
the masks' own error.  Between two chunkings the masks carry the fp32 U-Net bound (2e-5) and the waveform the transform bound (5e-5) of
tests/test_gpu_separate.py.  "both" against the single-output calls, and the rate conversion against the same steps by hand, are exact.
The path is not transparent at mask == 1 (forward n_fft 1023, inverse 1022): no test here expects an identity.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import separate_binaural_ref as BREF
import separate_ref as REF
from m2h import _lib, ops, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def policy_sd():
    return synthetic.make_state_dict(synthetic.policy_shapes(), SEED)


def _separator(sd, dev, math, **kw):
    from m2h.separate import Separator
    return Separator(sd, dev, math=math, **kw)


@pytest.fixture(scope="module")
def sep32(policy_sd, dev):
    return _separator(policy_sd, dev, ops.MATH_FP32)


@functools.lru_cache(maxsize=None)
def _reference(L, seed, overlap):
    """(wave [2, 2, L], y [2, 2, L], masks [2, S, 512, 32, 2]) of the CPU statement for classes [4, 7]; computed once, read-only."""
    sd = REF.torch_state_dict(synthetic.make_state_dict(synthetic.policy_shapes(), SEED))
    wave = REF.tone_noise(2, L, seed)
    y, masks = BREF.separate(sd, wave, [4, 7], overlap)
    for a in (wave, y, masks):
        a.setflags(write=False)
    return wave, y, masks


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N", [1, 3])
def test_kernel_alone_is_one_multiply_per_element(dev, N):
    rng = np.random.default_rng(60 + N)
    spec = rng.standard_normal((N * 64, 1024)).astype(np.float32)
    masks = (rng.standard_normal((N, 512, 32, 2)) * 2.0).astype(np.float32)
    masks[rng.random(masks.shape) < 0.1] = 0.0
    # rows [(n*2 + c)*32 + t][part*512 + k] = max(masks[n][k][t][c], 0) * spec[same]
    factor = np.maximum(masks, 0).transpose(0, 3, 2, 1)                       # [N, c, t, k]
    want = (factor[:, :, :, None, :] * spec.reshape(N, 2, 32, 2, 512)).reshape(N * 64, 1024)
    assert want.dtype == np.float32 and (want == 0).mean() > 0.5 and (want != 0).mean() > 0.3
    s, m = torch.from_numpy(spec).to(dev), torch.from_numpy(masks).to(dev)
    out = torch.full_like(s, float("nan"))
    got = ops.sep_bin_rows(s, m, out=out)
    assert got is out and torch.equal(s.cpu(), torch.from_numpy(spec)) and torch.equal(m.cpu(), torch.from_numpy(masks))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    inplace = s.clone()
    got = ops.sep_bin_rows(inplace, m)
    assert got is inplace and got.data_ptr() == inplace.data_ptr()
    assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want))
    with pytest.raises(RuntimeError, match="sep_bin_rows"):
        ops.sep_bin_rows(s[:-1], m)
    with pytest.raises(RuntimeError, match="sep_bin_rows"):
        ops.sep_bin_rows(s, m[:, :, :, :1].contiguous())
    with pytest.raises(RuntimeError, match="sep_bin_rows"):
        ops.sep_bin_rows(s, m, out=torch.empty((N * 32, 1024), device=dev))


@pytest.mark.parametrize("math", [ops.MATH_FP32, ops.MATH_BF16X3], ids=["fp32", "bf16x3"])
def test_end_to_end_matches_reference(dev, policy_sd, math):
    R, L = 2, 40000
    wave, want_y, want_m = _reference(L, 41, 1)
    # the inputs, checked on the CPU statement's own masks: a degenerate mask cannot hide a failure
    for c in range(2):
        share = float((want_m[..., c] > 0).mean())
        assert 0.3 <= share <= 0.7, (c, share)
    assert want_m.min() < -1 and want_m.max() > 1
    X = REF.segment_stft(wave)
    assert not (X[-1][..., :15] == 0).any() and (X[-1][..., 17:] == 0).all()   # the cut last segment: 8000 samples, frames 17.. are empty
    sep = _separator(policy_sd, dev, math)
    w = torch.from_numpy(np.array(wave)).to(dev)
    y, masks = sep.separate(w, [4, 7], output="binaural", return_spectrograms=True)
    assert ops.math_mode() == ops.MATH_FP32            # the separator's arithmetic does not leak into the calling thread
    assert y.shape == (R, 2, L) and masks.shape == (R, 3, 512, 32, 2) and y.is_contiguous()
    e_y, e_m = REF.rel_l1(y.cpu().numpy(), want_y), REF.rel_l1(masks.cpu().numpy(), want_m)
    e_c = [REF.rel_l1(y[:, c].cpu().numpy(), want_y[:, c]) for c in range(2)]
    print("binaural end to end [%s]: rel-L1 waveform %.3e (left %.3e, right %.3e), masks %.3e, positive mask share left %.3f right %.3f, mask range %.1f .. %.1f"
          % ("fp32" if math == ops.MATH_FP32 else "bf16x3", e_y, e_c[0], e_c[1], e_m, (want_m[..., 0] > 0).mean(), (want_m[..., 1] > 0).mean(),
             want_m.min(), want_m.max()))
    assert torch.isfinite(y).all()
    assert e_y <= 1e-3 and e_m <= 1e-3 and max(e_c) <= 1e-3
    # the last segment's empty frames are exactly zero in X and come out exactly zero, whatever their masks
    with ops.math_scope(math):
        spec = ops.linear(ops.sep_frames(w, sep._win_fwd, 2, 1), sep._W_fwd, None, name="test.dft")
        rows = ops.sep_bin_rows(spec, masks[:, 2].contiguous()).cpu().numpy().reshape(R, 2, 32, 1024)
    assert (rows[:, :, 17:] == 0).all() and (rows[:, :, :15] != 0).mean() > 0.3
    # the default (use_memory=None) and an explicit False are the same call
    assert torch.equal(sep.separate(w, [4, 7], output="binaural", use_memory=False), y)


def test_both_is_the_two_single_calls(dev, policy_sd, sep32):
    lib = _lib.load()
    R, L = 2, 40000
    w = torch.from_numpy(REF.tone_noise(R, L, 41)).to(dev)
    tc = [4, 7]
    assert sep32.memory is not None
    mono = sep32.separate(w, tc)                                   # memory on: the checkpoint has one
    n0 = lib.m2h_launch_count()
    bina = sep32.separate(w, tc, output="binaural")
    n1 = lib.m2h_launch_count()
    m2, b2 = sep32.separate(w, tc, output="both")
    assert m2.shape == (R, L) and b2.shape == (R, 2, L)
    assert torch.equal(m2, mono) and torch.equal(b2, bina)
    assert not torch.equal(mono, sep32.separate(w, tc, use_memory=False))     # and the memory took part in it
    m3, b3, P, ph, masks = sep32.separate(w, tc, output="both", return_spectrograms=True)
    y1, P1, ph1 = sep32.separate(w, tc, return_spectrograms=True)
    _, masks1 = sep32.separate(w, tc, output="binaural", return_spectrograms=True)
    assert P.shape == (R, 3, 512, 32) and ph.shape == (R, 3, 512, 32, 2) and masks.shape == (R, 3, 512, 32, 2)
    assert torch.equal(m3, mono) and torch.equal(b3, bina) and torch.equal(y1, mono)
    assert torch.equal(P, P1) and torch.equal(ph, ph1) and torch.equal(masks, masks1)
    # the binaural call runs one U-Net and no memory: fewer launches than the mono call
    n2 = lib.m2h_launch_count()
    sep32.separate(w, tc)
    n3 = lib.m2h_launch_count()
    assert n1 - n0 < n3 - n2
    assert ops.math_mode() == ops.MATH_FP32


def test_chunking_does_not_change_the_result(dev, policy_sd, sep32):
    R, L = 2, 40000
    w = torch.from_numpy(REF.tone_noise(R, L, 43)).to(dev)
    tc = [4, 7]
    ya, ma = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=2).separate(w, tc, output="binaural", return_spectrograms=True)
    yb, mb = sep32.separate(w, tc, output="binaural", return_spectrograms=True)
    e_m, e_y = REF.rel_l1(ma.cpu().numpy(), mb.cpu().numpy()), REF.rel_l1(ya.cpu().numpy(), yb.cpu().numpy())
    print("binaural, chunks of 1 segment x 2 recordings against one chunk: rel-L1 masks %.3e waveform %.3e" % (e_m, e_y))
    assert ma.shape == (R, 3, 512, 32, 2) and torch.isfinite(ya).all()
    assert e_m <= 2e-5 and e_y <= 5e-5


@pytest.mark.parametrize("overlap,max_segments,S", [(2, 4, 3), (4, 8, 5)])
def test_overlap_in_two_chunks_matches_reference(dev, policy_sd, overlap, max_segments, S):
    from m2h.separate import overlap_plan
    R, L = 2, 20000
    assert len(overlap_plan(L, overlap, max_segments // R)) == 2
    wave, want_y, want_m = _reference(L, 46, overlap)
    sep = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=max_segments)
    y, masks = sep.separate(torch.from_numpy(np.array(wave)).to(dev), [4, 7], output="binaural", return_spectrograms=True, overlap=overlap)
    assert y.shape == (R, 2, L) and masks.shape == want_m.shape == (R, S, 512, 32, 2)
    e_y, e_m = REF.rel_l1(y.cpu().numpy(), want_y), REF.rel_l1(masks.cpu().numpy(), want_m)
    print("binaural overlap %d, %d segments in two chunks: rel-L1 waveform %.3e, masks %.3e" % (overlap, S, e_y, e_m))
    assert torch.isfinite(y).all() and np.isfinite(want_y).all()
    assert e_y <= 1e-3 and e_m <= 1e-3


def test_rate_conversion_is_the_same_steps_by_hand(dev, sep32):
    rate, L = 44100, 30000
    w = torch.from_numpy(REF.tone_noise(1, L, 47)[0]).to(dev)          # [2, L]
    y = sep32.separate(w, 4, output="binaural", sample_rate=rate)
    assert y.shape == (2, L) and torch.isfinite(y).all() and float(y.abs().max()) > 0
    to16, back = sep32.resamplers(rate)
    y16 = sep32.separate(to16(w.unsqueeze(0)), 4, output="binaural")
    want = back(y16)[:, :, :L].contiguous()[0]
    assert torch.equal(y, want)


def test_cut_off_length_and_target_class(dev, sep32):
    L = 16001
    w = torch.from_numpy(REF.tone_noise(1, L, 48)[0]).to(dev)          # [2, L]
    a = sep32.separate(w, 4, output="binaural")
    b = sep32.separate(w, 7, output="binaural")
    assert a.shape == (2, L) and b.shape == (2, L) and torch.isfinite(a).all() and torch.isfinite(b).all()
    change = REF.rel_l1(b.cpu().numpy(), a.cpu().numpy())
    print("binaural, target class 4 -> 7: rel change %.3f" % change)
    assert change > 0.1


def test_argument_errors_come_before_any_gpu_work(dev, sep32):
    lib = _lib.load()
    w = torch.from_numpy(REF.tone_noise(1, 16000, 49)).to(dev)
    n0 = lib.m2h_launch_count()
    for bad in ("stereo", "", None, 1, "Mono"):
        with pytest.raises(ValueError, match="output"):
            sep32.separate(w, 4, output=bad)
    with pytest.raises(ValueError, match="memory"):
        sep32.separate(w, 4, output="binaural", use_memory=True)
    assert lib.m2h_launch_count() == n0


def test_cli_both(dev, policy_sd, sep32, tmp_path):
    from scipy.io import wavfile
    L = 20000
    wave = REF.tone_noise(1, L, 45)[0]                 # [2, L]
    samples = np.clip(np.rint(wave.T * 32768.0), -32768, 32767).astype(np.int16)
    as_float = np.ascontiguousarray(samples.astype(np.float32).T * np.float32(1.0 / 32768.0))
    inp, out, outb, ckpt = (str(tmp_path / n) for n in ("mix.wav", "mono.wav", "bin.wav", "ckpt.pth"))
    wavfile.write(inp, 16000, samples)
    torch.save({"state_dict": {"actor_critic." + k: torch.from_numpy(np.asarray(v)) for k, v in policy_sd.items()}, "config": {}}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "separate.py"), "--ckpt", ckpt, "--in", inp, "--target-class", "5", "--out", out, "--math", "fp32"]
    # one without the other is an error of the command line, before anything is loaded
    for extra in (["--output", "both"], ["--out-binaural", outb], ["--output", "binaural", "--out-binaural", outb]):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode != 0 and "--out-binaural" in r.stdout and not os.path.exists(out) and not os.path.exists(outb)
    r = subprocess.run(cmd + ["--output", "both", "--out-binaural", outb], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    rate, mono = wavfile.read(out)
    rate_b, bina = wavfile.read(outb)
    assert rate == 16000 and mono.shape == (L,) and mono.dtype == np.int16
    assert rate_b == 16000 and bina.shape == (L, 2) and bina.dtype == np.int16
    ym, yb = sep32.separate(torch.from_numpy(as_float).to(dev), 5, output="both")

    def to_int16(a):
        return np.clip(np.rint(a.cpu().numpy().astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(mono, to_int16(ym)) and np.array_equal(bina, to_int16(yb).T)
    assert np.abs(bina).max() > 0 and not np.array_equal(bina[:, 0], bina[:, 1])
