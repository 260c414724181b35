"""GPU: a recording pushed block by block (Separator.stream, ResamplerStream, the window kernels of csrc/separate.hip and
csrc/resample.hip) against the one-call path on the same recording -- no other oracle: what separate() promises is stated in
m2h/separate.py and checked by tests/test_gpu_separate*.py.

Bit for bit wherever the stream runs the same rows through the same kernels (the rate conversion for any blocking, the window kernels,
overlap 1 with one segment per push against max_segments = R, overlap 2 and 4 with the pushes that complete overlap_plan's chunks).  Where the blocking changes the U-Nets' batch size the bound is the
existing one for "the same rows at another batch size" (tests/test_gpu_separate.py): 2e-5 on P, times 2.5, plus 5e-5 = 1e-4 on the
waveform in fp32, and the project's 1e-3 parity contract in bf16x3.  Weights and inputs as tests/test_gpu_separate.py.
Measured on MI355X: DESIGN.md section 8.4.
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
from m2h.audio.resample import Resampler, ready_outputs
from m2h.separate import Separator, stream_emitted, stream_returned

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2
SEG = 16000
TC = [4, 7]
BOUND = 1e-4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def policy_sd():
    return synthetic.make_state_dict(synthetic.policy_shapes(), SEED)


@functools.lru_cache(maxsize=None)
def _sep(math=ops.MATH_FP32, max_segments=None):
    sd = synthetic.make_state_dict(synthetic.policy_shapes(), SEED)
    kw = {} if max_segments is None else {"max_segments": max_segments}
    return Separator(sd, torch.device("cuda", 0), math=math, **kw)


@functools.lru_cache(maxsize=None)
def _wave(R, L, seed):
    return torch.from_numpy(REF.tone_noise(R, L, seed)).to(torch.device("cuda", 0))


def _blocks(L, sizes):
    """The given block sizes, cut where the recording ends, then the rest."""
    out, a = [], 0
    for n in sizes:
        n = min(n, L - a)
        out.append((a, a + n))
        a += n
    out.append((a, L))
    return out


def _run_stream(st, wave, sizes, check=None):
    """Push wave [R, 2, L] in blocks, flush; returns the concatenated result(s) as a tuple.  check(P, E): called after every push."""
    parts, P, E = [], 0, 0
    for a, b in _blocks(wave.shape[-1], sizes):
        res = st.push(wave[:, :, a:b].contiguous())
        res = res if isinstance(res, tuple) else (res,)
        parts.append(res)
        P, E = b, E + res[0].shape[-1]
        assert all(r.shape[-1] == res[0].shape[-1] for r in res)
        if check is not None:
            check(P, E)
    res = st.flush()
    parts.append(res if isinstance(res, tuple) else (res,))
    return tuple(torch.cat([p[i] for p in parts], dim=-1) for i in range(len(parts[0])))


# ---- 1. the rate conversion, bit for bit for any blocking
@pytest.mark.parametrize("f_in,f_out,L,kernel", [(44100, 16000, 5003, "resample_poly_win"), (16000, 44100, 2001, "resample_poly_win"),
                                                 (48000, 16000, 4801, "resample_poly_win"), (16000, 48000, 1601, "resample_poly_win"),
                                                 (1023, 1000, 3000, "resample_poly_win_direct")])
def test_resampler_stream_is_the_one_call_result_bit_for_bit(dev, f_in, f_out, L, kernel):
    rs = Resampler(f_in, f_out, dev)
    x = torch.from_numpy(RR.tone_noise(3, L, 100 + L % 97, f_in)).to(dev)
    want = rs(x)
    st = rs.stream((3,))
    parts, P, E = [], 0, 0
    for a, b in _blocks(L, (1, 2, 0, 499, 1500)):
        y = st.push(x[:, a:b].contiguous())
        P, E = b, E + y.shape[1]
        assert y.shape[0] == 3 and E == ready_outputs(P, rs.up, rs.down) == st.emitted, (P, E)
        if y.shape[1]:
            assert ops.last_kernel() == kernel
        parts.append(y)
    parts.append(st.flush())
    got = torch.cat(parts, dim=1)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert torch.equal(got, want)
    with pytest.raises(RuntimeError, match="after flush"):
        st.push(x[:, :1].contiguous())
    st.reset()
    again = torch.cat([st.push(x[:, :L // 2].contiguous()), st.push(x[:, L // 2:].contiguous()), st.flush()], dim=1)    # the same buffers, another blocking
    assert torch.equal(again, want)


# ---- 2. the window kernels, bit for bit
@pytest.fixture(scope="module")
def transforms(dev):
    from m2h.audio.stft import ISTFT, STFT
    from m2h.separate import crossfade_window
    fwd, inv = STFT(dev), ISTFT(dev)
    return torch.cat((fwd.window, torch.zeros(1, device=dev))), inv.window, torch.from_numpy(crossfade_window()).to(dev)


def test_frames_from_a_window(dev, transforms):
    win = transforms[0]
    R, L, hop, origin, cap = 2, 24001, 4000, 8000, 16004
    wave = _wave(R, L, 21)
    buf = torch.full((R, 2, cap), float("nan"), device=dev)
    buf[:, :, :L - origin] = wave[:, :, origin:]
    want = ops.sep_frames(wave, win, 2, 5, hop=hop)                      # segments 2 .. 6, the last one cut after one sample
    got = ops.sep_frames(buf, win, 2, 5, hop=hop, origin=origin, end=L)
    assert ops.last_kernel() == "sep_frames_win"
    assert torch.isfinite(got).all() and torch.equal(got, want)
    # an earlier `end`: the samples from there on are zero, as in a recording that ends there
    short = ops.sep_frames(buf, win, 2, 4, hop=hop, origin=origin, end=20001)
    assert torch.equal(short, ops.sep_frames(wave[:, :, :20001].contiguous(), win, 2, 4, hop=hop))
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    with pytest.raises(RuntimeError, match="leave the window"):
        ops.sep_frames(buf, win, 1, 2, hop=hop, origin=origin, end=L)    # segment 1 starts at 4000, before the window
    assert lib.m2h_launch_count() == n0


@pytest.mark.parametrize("L,k", [(24001, 4), (16001, 1)])
def test_inverse_into_a_sliding_window(dev, transforms, L, k):
    """One segment per call, the window moved by one hop between calls: the cross-fade (k = 4) and the plain overlap-add (k = 1)."""
    _, win, xwin = transforms
    R, H, cap = 3, SEG // k, SEG
    S = -(-L // H)
    g = torch.Generator(device="cpu").manual_seed(31)
    frames = torch.randn((S * R * 32, 1024), generator=g).to(dev)
    want = torch.full((R, L), float("nan"), device=dev)
    if k == 1:
        ops.sep_istft_ola(frames, win, want, 0, S)
    else:
        ops.sep_istft_xfade(frames, win, xwin, want, H, 0, S)
    y = torch.full((R, cap), float("nan"), device=dev)
    parts, rows = [], R * 32
    for s in range(S):
        origin = s * H
        end = origin + SEG if origin + SEG <= L else L                   # what has arrived when the segment is processed
        if s:
            moved = torch.full((R, cap), float("nan"), device=dev)
            moved[:, :cap - H] = y[:, H:]
            y = moved
        if k == 1:
            ops.sep_istft_ola(frames[s * rows:(s + 1) * rows], win, y, s, 1, origin=origin, end=end)
        else:
            ops.sep_istft_xfade(frames[s * rows:(s + 1) * rows], win, xwin, y, H, s, 1, origin=origin, end=end)
        parts.append(y[:, :(H if s < S - 1 else L - origin)].clone())
    got = torch.cat(parts, dim=1)
    assert got.shape == want.shape and torch.isfinite(got).all() and torch.isfinite(want).all()
    assert torch.equal(got, want)


# ---- 3. end to end, overlap 1, one segment per push: the same batches through the same kernels
@pytest.mark.parametrize("use_memory", [True, False], ids=["memory", "nomemory"])
def test_overlap_one_is_bit_identical(dev, use_memory):
    R, L = 2, 50001
    wave = _wave(R, L, 41)
    sep = _sep(ops.MATH_FP32, R)
    want = sep.separate(wave, TC, use_memory=use_memory)
    st = sep.stream(TC, recordings=R, use_memory=use_memory)

    def check(P, E):
        assert E == stream_emitted(P, 1), (P, E)

    (got,) = _run_stream(st, wave, (1, 15999, 7000, 9000, 16000, 2001), check)     # cut at L: no push completes two segments
    assert got.shape == (R, L) and torch.isfinite(got).all()
    assert ops.math_mode() == ops.MATH_FP32
    assert torch.equal(got, want)


# ---- 4. any blocking, overlap 2 and 4
@functools.lru_cache(maxsize=None)
def _offline(math, L, seed, use_memory, overlap, output="mono", rate=16000):
    return _sep(math).separate(_wave(2, L, seed), TC, use_memory=use_memory, overlap=overlap, output=output, sample_rate=rate)


@pytest.mark.parametrize("overlap,use_memory,math,bound", [(2, True, ops.MATH_FP32, BOUND), (4, False, ops.MATH_FP32, BOUND), (2, True, ops.MATH_BF16X3, 1e-3)],
                         ids=["k2-memory-fp32", "k4-nomemory-fp32", "k2-memory-bf16x3"])
def test_any_blocking_with_overlap(dev, overlap, use_memory, math, bound):
    R, L = 2, 52001
    wave = _wave(R, L, 43)
    want = _offline(math, L, 43, use_memory, overlap)
    st = _sep(math).stream(TC, recordings=R, use_memory=use_memory, overlap=overlap)

    def check(P, E):
        assert E == stream_emitted(P, overlap), (P, E)

    (got,) = _run_stream(st, wave, (5000, 33000, 1, 9000, 0, 4999), check)           # 33000: several segments in one push
    e = REF.rel_l1(got.cpu().numpy(), want.cpu().numpy())
    print("stream overlap %d, memory %s, %s: rel-L1 to separate() %.3e" % (overlap, "on" if use_memory else "off", "fp32" if math == ops.MATH_FP32 else "bf16x3", e))
    assert got.shape == (R, L) and torch.isfinite(got).all() and torch.isfinite(want).all()
    assert e < bound


@pytest.mark.parametrize("overlap,sizes", [(2, (24000, 16000, 4001)), (4, (28000, 16000, 1))], ids=["k2", "k4"])
def test_same_batches_with_overlap_are_bit_identical(dev, overlap, sizes):
    """The pushes and the flush complete segments [0, k), [k, 2k), [2k, 3k): overlap_plan(44001, k, k), the batches separate() runs
    at max_segments = k * R, through the same chunk method, the same kernels and the same memory steps."""
    R, L = 2, 44001
    wave = _wave(R, L, 53)
    sep = _sep(ops.MATH_FP32, overlap * R)
    want = sep.separate(wave, TC, use_memory=True, overlap=overlap)
    st = sep.stream(TC, recordings=R, use_memory=True, overlap=overlap)
    batches = []

    def check(P, E):
        assert E == stream_emitted(P, overlap), (P, E)
        batches.append(st.next_seg)

    (got,) = _run_stream(st, wave, sizes, check)
    assert batches == [overlap, 2 * overlap, 2 * overlap, 2 * overlap] and st.next_seg == 3 * overlap     # (the last push of _run_stream is empty)
    assert got.shape == (R, L) and torch.isfinite(got).all()
    assert torch.equal(got, want)


# ---- 5. other sample rates
@pytest.mark.parametrize("rate", [44100, 8000])
def test_other_sample_rates(dev, rate):
    R, L = 2, rate * 8 // 5                               # 1.6 s
    wave = torch.from_numpy(RR.tone_noise(2 * R, L, 51, rate).reshape(R, 2, L)).to(dev)
    sep = _sep(ops.MATH_FP32)
    want = sep.separate(wave, TC, use_memory=False, sample_rate=rate)
    st = sep.stream(TC, recordings=R, use_memory=False, sample_rate=rate)
    worst = [0]

    def check(P, E):
        assert E == stream_returned(P, rate, 1), (P, E)
        assert 0 <= P - E <= 1.01 * rate, (P, E)
        worst[0] = max(worst[0], P - E)

    (got,) = _run_stream(st, wave, (1, rate // 3, 7, rate - 5, 0, rate // 10, 3), check)
    e = REF.rel_l1(got.cpu().numpy(), want.cpu().numpy())
    print("stream at %d Hz, L %d: rel-L1 to separate() %.3e, worst backlog %.4f s" % (rate, L, e, worst[0] / rate))
    assert got.shape == (R, L) and torch.isfinite(got).all()
    assert e < BOUND


# ---- 6. the binaural outputs
def test_binaural_and_both(dev):
    R, L, overlap = 2, 40000, 2
    wave = _wave(R, L, 45)
    sep = _sep(ops.MATH_FP32)
    sizes = (9000, 20000, 3, 7000)
    want_mono, want_bin = _offline(ops.MATH_FP32, L, 45, False, overlap, "both")
    (mono,) = _run_stream(sep.stream(TC, recordings=R, use_memory=False, overlap=overlap), wave, sizes)
    (binaural,) = _run_stream(sep.stream(TC, recordings=R, overlap=overlap, output="binaural"), wave, sizes)
    both = _run_stream(sep.stream(TC, recordings=R, use_memory=False, overlap=overlap, output="both"), wave, sizes)
    assert mono.shape == (R, L) and binaural.shape == (R, 2, L) and both[0].shape == (R, L) and both[1].shape == (R, 2, L)
    assert torch.equal(both[0], mono) and torch.equal(both[1], binaural)
    e_m, e_b = REF.rel_l1(mono.cpu().numpy(), want_mono.cpu().numpy()), REF.rel_l1(binaural.cpu().numpy(), want_bin.cpu().numpy())
    print("stream overlap 2: rel-L1 to separate() mono %.3e, binaural %.3e" % (e_m, e_b))
    assert torch.isfinite(binaural).all() and e_m < BOUND and e_b < BOUND
    with pytest.raises(ValueError, match="binaural"):
        sep.stream(TC, recordings=R, output="binaural", use_memory=True)
    # overlap 1: the output is written straight into the returned tensor, [2R, m] rows
    (b1,) = _run_stream(sep.stream(TC, recordings=R, output="binaural"), wave, sizes)
    e = REF.rel_l1(b1.cpu().numpy(), _offline(ops.MATH_FP32, L, 45, None, 1, "binaural").cpu().numpy())
    print("stream overlap 1 binaural: rel-L1 to separate() %.3e" % e)
    assert b1.shape == (R, 2, L) and e < BOUND


# ---- 7. stream state and argument errors
def test_streams_do_not_disturb_each_other_and_reset(dev):
    R, L = 2, 36001
    wave = _wave(R, L, 47)
    sep = _sep(ops.MATH_FP32)
    sizes = (16000, 4000, 12000)
    kw = dict(recordings=R, use_memory=True, overlap=2)
    a = sep.stream([4, 7], **kw)
    (solo_a,) = _run_stream(a, wave, sizes)
    (solo_b,) = _run_stream(sep.stream([9, 2], **kw), wave, sizes)
    assert not torch.equal(solo_a, solo_b)
    a.reset()
    b = sep.stream([9, 2], **kw)
    parts_a, parts_b = [], []
    for lo, hi in _blocks(L, sizes):                     # interleaved
        parts_a.append(a.push(wave[:, :, lo:hi].contiguous()))
        parts_b.append(b.push(wave[:, :, lo:hi].contiguous()))
    parts_b.append(b.flush())
    parts_a.append(a.flush())
    assert torch.equal(torch.cat(parts_a, dim=1), solo_a)                # and a ran after reset(): the first run again, exactly
    assert torch.equal(torch.cat(parts_b, dim=1), solo_b)
    with pytest.raises(RuntimeError, match="after flush"):
        a.push(wave[:, :, :10].contiguous())
    lib = _lib.load()
    st = sep.stream(4, recordings=R)
    n0 = lib.m2h_launch_count()
    empty = st.push(wave[:, :, :0].contiguous())
    assert empty.shape == (R, 0) and empty.dtype == torch.float32 and empty.device == wave.device
    for bad in (wave[:1, :, :100].contiguous(), wave[:, :, :100].double(), wave[:, :, :100].cpu(), wave[:, :1, :100].contiguous(), wave[0, :, :100].contiguous()):
        with pytest.raises(RuntimeError):
            st.push(bad)
    assert lib.m2h_launch_count() == n0
    tail = st.flush()
    assert tail.shape == (R, 0)                          # L = 0
    both = sep.stream(4, recordings=R, output="both", overlap=4, sample_rate=44100)
    m, bn = both.flush()
    assert m.shape == (R, 0) and bn.shape == (R, 2, 0)


# ---- 8. the command line
def test_cli_stream_block(dev, policy_sd, tmp_path):
    from scipy.io import wavfile
    L = 40000                                             # 2.5 s
    wave = REF.tone_noise(1, L, 49)[0]
    samples = np.clip(np.rint(wave.T * 32768.0), -32768, 32767).astype(np.int16)
    inp, out, out_s, ckpt = str(tmp_path / "mix.wav"), str(tmp_path / "out.wav"), str(tmp_path / "out_stream.wav"), str(tmp_path / "ckpt.pth")
    wavfile.write(inp, 16000, samples)
    torch.save({"state_dict": {"actor_critic." + k: torch.from_numpy(np.asarray(v)) for k, v in policy_sd.items()}, "config": {}}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "separate.py"), "--ckpt", ckpt, "--in", inp, "--target-class", "5", "--math", "fp32", "--overlap", "2"]
    procs = [subprocess.Popen(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for extra in (["--out", out], ["--out", out_s, "--stream-block", "5000"])]
    for p in procs:
        text, _ = p.communicate(timeout=600)
        assert p.returncode == 0, text
    assert "blocks of 5000" in text
    (rate_a, a), (rate_b, b) = wavfile.read(out), wavfile.read(out_s)
    assert rate_a == rate_b == 16000 and a.shape == b.shape == (L,) and a.dtype == b.dtype == np.int16
    # the float values agree to the bound of test 4; rounding to int16 may then differ by one step
    diff = np.abs(a.astype(np.int64) - b.astype(np.int64))
    print("cli --stream-block: max |difference| %d steps, mean %.3e" % (diff.max(), diff.mean()))
    assert np.abs(a).max() > 0
    assert np.abs(diff - np.minimum(diff, 1)).sum() / max(np.abs(a.astype(np.float64)).sum(), 1e-30) < BOUND
