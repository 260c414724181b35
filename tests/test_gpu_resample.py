"""GPU: the polyphase rate conversion (csrc/resample.hip, m2h.audio.resample) against scipy.signal.resample_poly in float64, and
Separator / separate.py at other sample rates against scipy -> tests/separate_ref.py -> scipy.

Bounds.  The kernel: rel-L1 < 2e-5 over all rows, the bound tests/test_gpu_separate.py puts on the fp32 STFT glue whose sums are 18
times longer; rounding input and taps to fp32 costs 3-7e-8, and a real defect costs far more (one dropped tap 3.5e-4, taps shifted by
one 3.9e-3 on the CPU restatement: test_bound_discriminates asserts that both fail the bound).  End to end: rel-L1 <= 1e-3, the
project's parity contract, as the existing end-to-end tests.

Measured on MI355X: the figures are in DESIGN.md section 8.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_ref as RR
import separate_ref as REF
from m2h import _lib, ops, synthetic
from m2h.audio.resample import Resampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5
LENGTHS = [1, 5, 1023, 4096, 30001, 70003]       # shorter than one tap set; unaligned row bases; L % 4 == 0; several workgroup tiles
SEED = 2


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _resampler(f_in, f_out):
    return Resampler(f_in, f_out, torch.device("cuda", 0))


def _gpu(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)          # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def _case(f_in, f_out, L, rows=6):
    """(input fp32, scipy's float64 result): computed once per case"""
    up, down = RR.ratio(f_in, f_out)
    x = RR.tone_noise(rows, L, 100 + L % 97, f_in)
    want = RR.scipy_resample(x, up, down)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("f_in,f_out", RR.RATES)
def test_kernel_matches_scipy(dev, f_in, f_out, L):
    rs = _resampler(f_in, f_out)
    x, want = _case(f_in, f_out, L)
    T = RR.TAPS[(f_in, f_out)]
    assert rs.T == T and tuple(rs.table.shape) == (rs.up, T)
    y = rs(_gpu(x, dev).reshape(3, 2, L))          # R = 3 recordings x 2 channels
    assert y.shape == (3, 2, want.shape[1]) and ops.last_kernel() == "resample_poly"
    got = y.reshape(6, -1).cpu().numpy()
    e = RR.rel_l1(got, want)
    e_head, e_tail = RR.rel_l1(got[:, :T], want[:, :T]), RR.rel_l1(got[:, -T:], want[:, -T:])      # the zero extension at both ends
    print("resample %d -> %d, L_in %d -> %d: rel-L1 %.3e (first %d outputs %.3e, last %.3e)" % (f_in, f_out, L, want.shape[1], e, T, e_head, e_tail))
    assert np.isfinite(got).all()
    assert e < BOUND and e_head < BOUND and e_tail < BOUND


# the ratios at which the launch takes another kernel: tiles of 1024 / 512 / 256 outputs (the span of a larger tile does not fit
# into LDS), with one phase and with a table, and the kernel without staging for ratios whose table or span never fits
OTHER_KERNELS = [(128000, 16000, "resample_poly"), (256000, 16000, "resample_poly"), (512000, 16000, "resample_poly"),
                 (32000, 3000, "resample_poly"), (1000, 1, "resample_poly_direct"), (1023, 1000, "resample_poly_direct"),
                 (1000, 1023, "resample_poly_direct")]


@pytest.mark.parametrize("f_in,f_out,kernel", OTHER_KERNELS)
def test_every_kernel_variant_matches_scipy(dev, f_in, f_out, kernel):
    rs = _resampler(f_in, f_out)
    for L in (5, 30001):
        x, want = _case(f_in, f_out, L, 3)
        got = rs(_gpu(x, dev))
        assert ops.last_kernel() == kernel
        e = RR.rel_l1(got.cpu().numpy(), want)
        print("resample %d -> %d (%d/%d), L_in %d -> %d [%s]: rel-L1 %.3e" % (f_in, f_out, rs.up, rs.down, L, want.shape[1], kernel, e))
        assert got.shape == want.shape and e < BOUND


def test_bound_discriminates():
    """On the CPU restatement at 44100 -> 16000, L = 3000: one dropped tap and taps shifted by one both miss the bound."""
    up, down, half, h = RR.taps(44100, 16000)
    x = RR.tone_noise(2, 3000, 5, 44100)
    want = RR.scipy_resample(x, up, down)
    assert RR.rel_l1(RR.polyphase(x, h, up, down, half), want) < 1e-12
    dropped = h.copy()
    dropped[half + 3 * up] = 0.0
    shifted = np.concatenate((h[1:], [0.0]))
    e_drop = RR.rel_l1(RR.polyphase(x, dropped, up, down, half), want)
    e_shift = RR.rel_l1(RR.polyphase(x, shifted, up, down, half), want)
    print("mutated references: one dropped tap %.3e, taps shifted by one %.3e (bound %.0e)" % (e_drop, e_shift, BOUND))
    assert e_drop > BOUND and e_shift > BOUND


@pytest.mark.parametrize("f_in,f_out", [(48000, 16000), (44100, 16000), (16000, 44100), (1023, 1000)])
def test_rows_are_isolated(dev, f_in, f_out):
    rs = _resampler(f_in, f_out)
    x = torch.full((4, 10007), 1e6, device=dev)
    x[0] = 0.0
    x[2] = 0.0
    y = rs(x)
    assert torch.count_nonzero(y[0]) == 0 and torch.count_nonzero(y[2]) == 0
    assert torch.isfinite(y).all() and float(y[1].abs().max()) > 1e5 and torch.equal(y[1], y[3])


def test_long_recording_index_arithmetic(dev):
    """One row of 13.5 M samples at 44.1 kHz: n * down passes 2^31 near the end."""
    f_in, f_out, L = 44100, 16000, 13500000
    up, down, half, h = RR.taps(f_in, f_out)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, L), dtype=np.float32) * np.float32(0.05)
    x[0, -400000:] += (0.3 * np.sin(2 * np.pi * 440.0 / f_in * np.arange(400000))).astype(np.float32)
    Lo = RR.out_len(L, up, down)
    assert (Lo - 1) * down > 2 ** 31
    y = _resampler(f_in, f_out)(torch.from_numpy(x).to(dev))
    assert y.shape == (1, Lo) and bool(torch.isfinite(y).all())
    for lo, hi in ((0, 1000), (Lo - 100000, Lo)):
        want = RR.polyphase(x, h, up, down, half, lo, hi)
        e = RR.rel_l1(y[:, lo:hi].cpu().numpy(), want)
        print("long row, outputs [%d, %d) of %d: rel-L1 %.3e" % (lo, hi, Lo, e))
        assert e < BOUND


def test_two_calls_give_the_same_bits(dev):
    for f_in, f_out in ((44100, 16000), (16000, 44100), (48000, 16000)):
        x = _gpu(_case(f_in, f_out, 70003)[0], dev)
        rs = _resampler(f_in, f_out)
        assert torch.equal(rs(x), rs(x))


# ---- Separator and separate.py at other sample rates

@pytest.fixture(scope="module")
def policy_sd():
    return synthetic.make_state_dict(synthetic.policy_shapes(), SEED)


@functools.lru_cache(maxsize=None)
def _e2e_reference(rate, L):
    """scipy down -> tests/separate_ref.py -> scipy up, cut at L (memory off, R = 2)"""
    sd = REF.torch_state_dict(synthetic.make_state_dict(synthetic.policy_shapes(), SEED))
    wave = RR.tone_noise(4, L, 51, rate).reshape(2, 2, L)
    a, b = RR.ratio(rate, 16000)
    wave16 = RR.scipy_resample(wave, a, b).astype(np.float32)
    y16, P, _ = REF.separate(sd, wave16, [4, 7], use_memory=False)
    y = RR.scipy_resample(y16, b, a)
    assert y.shape[1] >= L
    return wave, y[:, :L], P


@pytest.mark.parametrize("math", [ops.MATH_FP32, ops.MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("rate,L", [(44100, 70003), (48000, 50001)])
def test_end_to_end_at_other_rates(dev, policy_sd, math, rate, L):
    from m2h.separate import Separator
    wave, want_y, want_P = _e2e_reference(rate, L)
    sep = Separator(policy_sd, dev, math=math)
    y, P, ph = sep.separate(torch.from_numpy(wave).to(dev), [4, 7], use_memory=False, return_spectrograms=True, sample_rate=rate)
    S = want_P.shape[1]
    assert y.shape == (2, L) and y.is_contiguous() and P.shape == (2, S, 512, 32) and ph.shape == (2, S, 512, 32, 2)
    assert ops.math_mode() == ops.MATH_FP32
    e_y, e_P = REF.rel_l1(y.cpu().numpy(), want_y), REF.rel_l1(P.cpu().numpy(), want_P)
    print("end to end at %d Hz [%s], L %d: rel-L1 waveform %.3e, P %.3e" % (rate, "fp32" if math == ops.MATH_FP32 else "bf16x3", L, e_y, e_P))
    assert torch.isfinite(y).all()
    assert e_y <= 1e-3 and e_P <= 1e-3
    assert sep.resamplers(rate) is sep.resamplers(rate) and list(sep._resamplers) == [rate]      # one pair per rate, kept
    y1 = sep.separate(torch.from_numpy(wave[0]).to(dev), 4, use_memory=False, sample_rate=rate)   # the [2, L] form
    assert y1.shape == (L,)
    with pytest.raises(ValueError, match="16001"):
        sep.separate(torch.from_numpy(wave).to(dev), 4, sample_rate=16001)


def test_sixteen_kilohertz_is_the_unchanged_path(dev, policy_sd):
    from m2h.separate import Separator
    lib = _lib.load()
    wave = torch.from_numpy(REF.tone_noise(2, 24001, 52)).to(dev)
    sep = Separator(policy_sd, dev, math=ops.MATH_FP32)
    sep.separate(wave, [4, 7])                           # the first call also packs the weights
    n0 = lib.m2h_launch_count()
    a = sep.separate(wave, [4, 7])
    n1 = lib.m2h_launch_count()
    b = sep.separate(wave, [4, 7], sample_rate=16000)
    n2 = lib.m2h_launch_count()
    assert torch.equal(a, b) and n2 - n1 == n1 - n0 and not sep._resamplers


def test_cli_resample(dev, policy_sd, tmp_path):
    from scipy.io import wavfile
    from m2h.separate import Separator
    L, rate = 50000, 44100
    wave = RR.tone_noise(2, L, 53, rate)
    samples = np.clip(np.rint(wave.T * 32768.0), -32768, 32767).astype(np.int16)
    as_float = np.ascontiguousarray(samples.astype(np.float32).T * np.float32(1.0 / 32768.0))
    inp, out, ckpt = str(tmp_path / "mix.wav"), str(tmp_path / "out.wav"), str(tmp_path / "ckpt.pth")
    wavfile.write(inp, rate, samples)
    torch.save({"state_dict": {"actor_critic." + k: torch.from_numpy(np.asarray(v)) for k, v in policy_sd.items()}, "config": {}}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "separate.py"), "--ckpt", ckpt, "--in", inp, "--target-class", "5", "--out", out, "--math", "fp32"]
    r = subprocess.run(cmd + ["--resample"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    got_rate, got = wavfile.read(out)
    assert got_rate == rate and got.shape == (L,) and got.dtype == np.int16
    y = Separator(policy_sd, dev, math=ops.MATH_FP32).separate(torch.from_numpy(as_float).to(dev), 5, sample_rate=rate).cpu().numpy()
    want = np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(got, want) and np.abs(got).max() > 0
    os.remove(out)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode != 0 and "16000" in r.stdout and "--resample" in r.stdout and not os.path.exists(out)
