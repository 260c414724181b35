"""GPU: m2h.separate with overlapped, cross-faded segments (overlap = k, H = 16000 / k) against its CPU reference
(tests/separate_overlap_ref.py: the cross-fade of tests/separate_ref.py on k shifted recordings).

Weights and inputs as tests/test_gpu_separate.py: synthetic.make_state_dict(synthetic.policy_shapes(), 2) and noise (sigma 0.05) plus
a tone, whose noise floor keeps the downmix phasor well conditioned.  No bin or sample is excluded from any comparison.

Bounds are those of the same arithmetic in tests/test_gpu_separate.py: 2e-5 magnitudes and 5e-5 complex values for framing + DFT +
post, 5e-5 for inverse + overlap-add (the cross-fade is a convex combination of such waveforms), rel-L1 <= 1e-3 end to end (the
project's parity contract), 2e-5 on P between two chunkings.  The result of the cross-fade kernel does not depend on the chunking at
all: every sample's additions have one fixed order.  Memory-on cases keep every chain at <= 4 steps: the synthetic memory weights are
not contractive.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_ref as RR
import separate_overlap_ref as OREF
import separate_ref as REF
from m2h import _lib, ops, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2
SEG = 16000


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def policy_sd():
    return synthetic.make_state_dict(synthetic.policy_shapes(), SEED)


@pytest.fixture(scope="module")
def transforms(dev):
    from m2h.audio.stft import ISTFT, STFT
    from m2h.separate import crossfade_window
    fwd, inv = STFT(dev), ISTFT(dev)
    win = torch.cat((fwd.window, torch.zeros(1, device=dev)))
    return fwd.W, win, inv.W, inv.window, torch.from_numpy(crossfade_window()).to(dev)


def _separator(sd, dev, math, **kw):
    from m2h.separate import Separator
    return Separator(sd, dev, math=math, **kw)


@pytest.mark.parametrize("hop,calls", [(8000, ((0, 3), (3, 1))), (4000, ((0, 2), (2, 5)))])
def test_frames_with_a_hop_match_np_stft_of_the_shifted_recordings(dev, transforms, hop, calls):
    Wf, win = transforms[:2]
    R, L = 2, 24001
    k = SEG // hop
    S = OREF.n_segments(L, k)
    wave = REF.tone_noise(R, L, 21)
    # [R, S, 2, 512, 32] in segment order: chain c is the plain segmentation of the recording from sample c * hop on
    X = OREF.interleave([REF.segment_stft(np.ascontiguousarray(wave[:, :, c * hop:])).transpose(1, 0, 2, 3, 4) for c in OREF.chains(L, k)], L, k)
    X = X.transpose(1, 0, 2, 3, 4)                                       # [S, R, 2, 512, 32]
    w = torch.from_numpy(wave).to(dev)
    parts = []
    assert sum(ns for _, ns in calls) == S
    for s0, ns in calls:
        frames = ops.sep_frames(w, win, s0, ns, hop=hop)
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
    print("frames_hop+post, hop %d: rel-L1 magnitudes %.3e, |X_left| * phasor %.3e, exactly-zero downmix bins %.1f %% (last segment %.1f %%)"
          % (hop, e_mag, e_z, 100 * zero.mean(), 100 * zero[-1].mean()))
    assert e_mag < 2e-5
    assert e_z < 5e-5
    # the last segment holds one sample: its all-zero frames give (1, 0) bit for bit
    assert zero[-1].mean() > 0.3 and np.all(ph[zero] == np.array([1.0, 0.0], np.float32))
    assert np.abs(np.abs(phc) - 1.0).max() < 1e-6


def _inverse_case(L, k, R=3, seed=31):
    """Random P (negative values included) and phasors with 10 % guarded bins for the S' segments, and the reference: the plain
    inverse of every chain, cross-faded in float64."""
    H = SEG // k
    S = OREF.n_segments(L, k)
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((S, R, 512, 32)) * 1.5).astype(np.float32)
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, (S, R, 512, 32)))
    ph[rng.random(ph.shape) < 0.1] = 1.0
    ph = ph.astype(np.complex64)
    want = OREF.crossfade([REF.inverse(P[c::k], ph[c::k].astype(np.complex128), L - c * H) for c in OREF.chains(L, k)], L, k)
    ph32 = np.stack((ph.real, ph.imag), -1).astype(np.float32)
    return P, ph32, want


def _inverse_frames(dev, Wi, P, ph32):
    S, R = P.shape[:2]
    rows = ops.sep_istft_pre(torch.from_numpy(P.reshape(S * R, 512, 32, 1)).to(dev), torch.from_numpy(ph32.reshape(S * R, 512, 32, 2)).to(dev))
    return ops.linear(rows, Wi, None, name="test.idft")                  # [S * R * 32, 1024], segment-major


@pytest.mark.parametrize("overlap", [2, 4])
@pytest.mark.parametrize("L", [24001, 32000, 4001, 3999])
def test_crossfade_kernel_matches_numpy(dev, transforms, L, overlap):
    _, _, Wi, win, xwin = transforms
    R = 3
    H = SEG // overlap
    S = OREF.n_segments(L, overlap)
    P, ph32, want = _inverse_case(L, overlap, R)
    y = torch.full((R, L), float("nan"), device=dev)
    for s0, ns in ((0, 1), (1, S - 1)) if S > 1 else ((0, 1),):         # two calls: the second adds onto what the first left
        frames = _inverse_frames(dev, Wi, P[s0:s0 + ns], ph32[s0:s0 + ns])
        ops.sep_istft_xfade(frames, win, xwin, y, H, s0, ns)
    y = y.cpu().numpy()
    e, e_head, e_tail = REF.rel_l1(y, want), REF.rel_l1(y[:, :16], want[:, :16]), REF.rel_l1(y[:, -16:], want[:, -16:])
    print("pre+xfade L=%d overlap=%d (%d segments): rel-L1 %.3e, first 16 samples %.3e, last 16 %.3e" % (L, overlap, S, e, e_head, e_tail))
    assert np.isfinite(y).all()
    assert e < 5e-5 and e_head < 5e-5 and e_tail < 5e-5


def test_crossfade_kernel_does_not_depend_on_the_chunking(dev, transforms):
    _, _, Wi, win, xwin = transforms
    R, L, overlap = 3, 24001, 4
    H = SEG // overlap
    P, ph32, _ = _inverse_case(L, overlap, R)
    frames = _inverse_frames(dev, Wi, P, ph32)                           # one GEMM: every chunking gets the same rows
    rows = R * 32
    outs = []
    for plan in (((0, 7),), ((0, 4), (4, 3)), tuple((s, 1) for s in range(7))):
        y = torch.full((R, L), float("nan"), device=dev)
        for s0, ns in plan:
            ops.sep_istft_xfade(frames[s0 * rows:(s0 + ns) * rows], win, xwin, y, H, s0, ns)
        outs.append(y)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


E2E_CASES = {"40000x2": (40000, 2, 41, 5), "24001x4": (24001, 4, 45, 7)}      # L, overlap, seed, S'


@functools.lru_cache(maxsize=None)
def _e2e_reference(case, use_memory):
    L, overlap, seed, _ = E2E_CASES[case]
    sd = REF.torch_state_dict(synthetic.make_state_dict(synthetic.policy_shapes(), SEED))
    wave = REF.tone_noise(2, L, seed)
    y, P, _ = OREF.separate(sd, wave, [4, 7], use_memory, overlap)
    for a in (wave, y, P):
        a.setflags(write=False)
    return wave, y, P


@pytest.mark.parametrize("math", [ops.MATH_FP32, ops.MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("use_memory", [True, False], ids=["memory", "nomemory"])
@pytest.mark.parametrize("case", sorted(E2E_CASES))
def test_end_to_end_matches_reference(dev, policy_sd, case, use_memory, math):
    L, overlap, _, S = E2E_CASES[case]
    wave, want_y, want_P = _e2e_reference(case, use_memory)
    sep = _separator(policy_sd, dev, math)
    y, P, ph = sep.separate(torch.from_numpy(np.array(wave)).to(dev), [4, 7], use_memory=use_memory, return_spectrograms=True, overlap=overlap)
    assert y.shape == (2, L) and P.shape == (2, S, 512, 32) and ph.shape == (2, S, 512, 32, 2)
    assert ops.math_mode() == ops.MATH_FP32            # the separator's arithmetic does not leak into the calling thread
    e_y, e_P = REF.rel_l1(y.cpu().numpy(), want_y), REF.rel_l1(P.cpu().numpy(), want_P)
    print("end to end %s [%s, memory %s]: rel-L1 waveform %.3e, P %.3e, max|y| %.2f (reference %.2f)"
          % (case, "fp32" if math == ops.MATH_FP32 else "bf16x3", "on" if use_memory else "off", e_y, e_P, float(y.abs().max()), np.abs(want_y).max()))
    assert torch.isfinite(y).all() and np.isfinite(want_y).all()
    assert e_y <= 1e-3 and e_P <= 1e-3


def test_overlap_changes_the_result_and_overlap_one_does_not(dev, policy_sd):
    lib = _lib.load()
    wave = torch.from_numpy(REF.tone_noise(2, 40000, 41)).to(dev)
    sep = _separator(policy_sd, dev, ops.MATH_FP32)
    sep.separate(wave, [4, 7])                                           # the first call also packs the weights, the memory's too
    a = sep.separate(wave, [4, 7], use_memory=False)
    b = sep.separate(wave, [4, 7], use_memory=False, overlap=2)
    change = REF.rel_l1(b.cpu().numpy(), a.cpu().numpy())
    print("overlap 1 -> 2: rel change %.3f" % change)
    assert change > 0.1
    n0 = lib.m2h_launch_count()
    c = sep.separate(wave, [4, 7])
    n1 = lib.m2h_launch_count()
    d = sep.separate(wave, [4, 7], overlap=1)
    n2 = lib.m2h_launch_count()
    assert torch.equal(c, d) and n2 - n1 == n1 - n0
    for bad in (0, 3, 8):
        with pytest.raises(ValueError, match="overlap"):
            sep.separate(wave, [4, 7], overlap=bad)
    assert lib.m2h_launch_count() == n2


def test_chunking_does_not_change_the_result(dev, policy_sd):
    R, overlap = 2, 2
    wave = torch.from_numpy(REF.tone_noise(R, 80000, 43)).to(dev)
    tc = [4, 7]
    ya, Pa, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=4).separate(wave, tc, use_memory=False, return_spectrograms=True, overlap=overlap)
    yb, Pb, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=64).separate(wave, tc, use_memory=False, return_spectrograms=True, overlap=overlap)
    e = REF.rel_l1(Pa.cpu().numpy(), Pb.cpu().numpy())
    print("overlap 2, chunks of 2 segments x 2 recordings against one chunk, 5 s, memory off: rel-L1 P %.3e waveform %.3e"
          % (e, REF.rel_l1(ya.cpu().numpy(), yb.cpu().numpy())))
    assert Pa.shape == (R, 10, 512, 32) and torch.isfinite(ya).all() and e < 2e-5
    # the two chains run across chunk borders: 7 segments as 4 + 3 against unchunked
    wave7 = wave[:, :, :56000].contiguous()
    yc, Pc, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=2 * R * 2).separate(wave7, tc, use_memory=True, return_spectrograms=True, overlap=overlap)
    yd, Pd, _ = _separator(policy_sd, dev, ops.MATH_FP32, max_segments=64).separate(wave7, tc, use_memory=True, return_spectrograms=True, overlap=overlap)
    e = REF.rel_l1(Pc.cpu().numpy(), Pd.cpu().numpy())
    print("overlap 2, memory on, 7 segments as 4 + 3 against unchunked: rel-L1 P %.3e waveform %.3e" % (e, REF.rel_l1(yc.cpu().numpy(), yd.cpu().numpy())))
    assert Pc.shape == (R, 7, 512, 32) and torch.isfinite(yc).all() and torch.isfinite(yd).all() and e < 2e-5
    assert REF.rel_l1(Pd[:, 4].cpu().numpy(), Pb[:, 4].cpu().numpy()) > 1e-2     # and the memory does something (segment 4: the same samples)


def test_rate_conversion_composes(dev, policy_sd):
    rate, L, overlap = 44100, 70003, 2
    sd = REF.torch_state_dict(policy_sd)
    wave = RR.tone_noise(4, L, 51, rate).reshape(2, 2, L)
    a, b = RR.ratio(rate, 16000)
    wave16 = RR.scipy_resample(wave, a, b).astype(np.float32)
    y16, want_P, _ = OREF.separate(sd, wave16, [4, 7], False, overlap)
    want_y = RR.scipy_resample(y16, b, a)[:, :L]
    sep = _separator(policy_sd, dev, ops.MATH_FP32)
    y, P, _ = sep.separate(torch.from_numpy(wave).to(dev), [4, 7], use_memory=False, return_spectrograms=True, sample_rate=rate, overlap=overlap)
    assert y.shape == (2, L) and P.shape == want_P.shape == (2, OREF.n_segments(wave16.shape[2], overlap), 512, 32)
    e_y, e_P = REF.rel_l1(y.cpu().numpy(), want_y), REF.rel_l1(P.cpu().numpy(), want_P)
    print("overlap 2 at %d Hz, L %d: rel-L1 waveform %.3e, P %.3e" % (rate, L, e_y, e_P))
    assert torch.isfinite(y).all()
    assert e_y <= 1e-3 and e_P <= 1e-3


def test_cli_overlap(dev, policy_sd, tmp_path):
    from scipy.io import wavfile
    L = 36000
    wave = REF.tone_noise(1, L, 45)[0]                 # [2, L]
    samples = np.clip(np.rint(wave.T * 32768.0), -32768, 32767).astype(np.int16)
    as_float = np.ascontiguousarray(samples.astype(np.float32).T * np.float32(1.0 / 32768.0))
    inp, out, ckpt = str(tmp_path / "mix.wav"), str(tmp_path / "out.wav"), str(tmp_path / "ckpt.pth")
    wavfile.write(inp, 16000, samples)
    torch.save({"state_dict": {"actor_critic." + k: torch.from_numpy(np.asarray(v)) for k, v in policy_sd.items()}, "config": {}}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "separate.py"), "--ckpt", ckpt, "--in", inp, "--target-class", "5", "--out", out, "--math", "fp32"]
    r = subprocess.run(cmd + ["--overlap", "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    rate, got = wavfile.read(out)
    assert rate == 16000 and got.shape == (L,) and got.dtype == np.int16
    sep = _separator(policy_sd, dev, ops.MATH_FP32)
    y = sep.separate(torch.from_numpy(as_float).to(dev), 5, overlap=2).cpu().numpy()
    want = np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(got, want) and np.abs(got).max() > 0
    plain = sep.separate(torch.from_numpy(as_float).to(dev), 5).cpu().numpy()
    assert not np.array_equal(want, np.clip(np.rint(plain.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16))
    os.remove(out)
    r = subprocess.run(cmd + ["--overlap", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode != 0 and "--overlap" in r.stdout and not os.path.exists(out)
