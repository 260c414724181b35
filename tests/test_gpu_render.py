"""GPU: m2h.audio.render (the Auralizer, csrc/render.hip) against its float64 definition (tests/render_ref.py).

Inputs: noise sources (sigma 0.1) and noise RIRs under an exponential envelope that falls to 1/30 at the last tap, R = 2.  Bounds, for
`images` and `mix`: rel-L1 < 2e-5, the project's bound for fp32 glue against float64 (test_gpu_separate.py, test_gpu_resample.py);
max|got - want| <= 2e-6 sqrt(15) * 2 Pn * T, m2h_fftconv_full's bound per product (test_gpu_feeder.py) times the at most 2 Pn products
over a sample, T the largest max-abs of any single block x partition convolution in float64 (for `mix` times sum_s |gains|); everything
finite.  tests/test_render_cpu.py shows what the rel-L1 bound rejects and what fp32 arithmetic costs.  Chunking, a repeated RIR, the
batch and `tail` do not change the arithmetic or its order: those comparisons are bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as REF
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 16000


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def aur(dev):
    from m2h.audio.render import Auralizer
    return Auralizer(dev)


_refs = {}


def reference(case):
    """(sources, rirs, mix, images, T) of a case: the float64 definition, evaluated once, shared and read-only"""
    if case not in _refs:
        x, h = REF.make_case(case)
        _refs[case] = (x, h) + REF.render_f64(x, h, tail=case[4]) + (REF.product_max(x, h),)
        for a in _refs[case][:4]:
            a.setflags(write=False)
    return _refs[case]


def _gpu(dev, *arrays):
    return [torch.tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]   # (a copy: the shared references are read-only)


def _assert_close(name, got, want, elem_bound):
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), name
    e = REF.rel_l1(got, want) if np.abs(want).sum() > 0 else float(np.abs(got).sum())
    d = np.abs(got - want).reshape(got.shape[0], -1).max(axis=1)
    print("%s: rel-L1 %.3e  max-abs %.3e of bound %.3e" % (name, e, d.max(), np.max(elem_bound)))
    assert e < REF.REL_L1_BOUND, (name, e)
    assert (d <= elem_bound).all(), (name, d, elem_bound)


@pytest.mark.parametrize("case", REF.CASES, ids=REF.case_id)
def test_render_matches_the_float64_definition(dev, aur, case):
    S, L, Lr, K, tail = case
    x, h, want_mix, want_images, T = reference(case)
    xs, hs = _gpu(dev, x, h if K > 1 else h[:, :, 0])                        # K = 1 in its four-axis form
    mix, images = aur.render(xs, hs, tail=tail, return_images=True)
    assert ops.last_kernel() == "render_mix"
    L_out = L + Lr - 1 if tail else L
    assert mix.shape == (REF.R, 2, L_out) and images.shape == (REF.R, S, 2, L_out)
    bound = REF.PRODUCT_BOUND * 2 * (-(-Lr // B)) * T
    _assert_close("images " + REF.case_id(case), images, want_images, bound)
    _assert_close("mix    " + REF.case_id(case), mix, want_mix, bound * np.abs(REF.default_gains(REF.R, S)).sum(axis=1))
    assert torch.equal(aur.render(xs, hs, tail=tail), mix)                    # without `images`: the same mixture


BIT_CASE = (3, 40001, 33000, 3, True)


def test_chunking_repeated_rir_batch_and_tail_are_bit_identical(dev):
    from m2h.audio.render import Auralizer
    S, L, Lr, K, _ = BIT_CASE
    x, h = REF.make_case(BIT_CASE)
    xs, hs = _gpu(dev, x, h)
    one = Auralizer(dev)
    mix, images = one.render(xs, hs, tail=True, return_images=True)
    for max_blocks in (1, 2):
        m2, i2 = Auralizer(dev, max_blocks=max_blocks).render(xs, hs, tail=True, return_images=True)
        assert torch.equal(m2, mix) and torch.equal(i2, images), max_blocks
    # the first L samples of tail=True are tail=False
    for max_blocks in (1, 1024):
        m3, i3 = Auralizer(dev, max_blocks=max_blocks).render(xs, hs, tail=False, return_images=True)
        assert m3.shape[-1] == L and torch.equal(m3, mix[..., :L]) and torch.equal(i3, images[..., :L])
    # each recording of the batch against its solo render
    for r in range(REF.R):
        m4, i4 = one.render(xs[r:r + 1].contiguous(), hs[r:r + 1].contiguous(), tail=True, return_images=True)
        assert torch.equal(m4[0], mix[r]) and torch.equal(i4[0], images[r])
    # K = J with the same RIR repeated against K = 1
    h1 = hs[:, :, 1].contiguous()
    m5, i5 = one.render(xs, h1, tail=True, return_images=True)
    m6, i6 = Auralizer(dev, max_blocks=2).render(xs, h1.unsqueeze(2).repeat(1, 1, K, 1, 1), tail=True, return_images=True)
    assert torch.equal(m5, m6) and torch.equal(i5, i6)
    assert not torch.equal(m5, mix)


def test_custom_gains(dev, aur):
    case = (3, 40001, 33000, 1, False)
    x, h, _, want_images, T = reference(case)
    gains = np.array([[0.7, 0.0, -1.5], [-0.25, 2.0, 0.0]], np.float32)
    xs, hs, gs = _gpu(dev, x, h, gains)
    mix, images = aur.render(xs, hs, gains=gs, return_images=True)
    bound = REF.PRODUCT_BOUND * 2 * 3 * T
    _assert_close("images, custom gains", images, want_images, bound)                      # unit gain whatever the mix uses
    _assert_close("mix, custom gains", mix, REF.mix_f64(want_images, gains), bound * np.abs(gains).sum(axis=1))


def test_kernel_labels(dev, aur):
    from m2h.audio.render import NFFT
    lib = _lib.load()
    x, h = _gpu(dev, REF.make_sources(1, 1, 100, 1), REF.make_rirs(1, 1, 1, 50, 1)[:, :, 0])
    tw = aur._twiddle_table()
    xspec, hspec = torch.empty((1, 1, NFFT), device=dev), torch.empty((1, 1, 2, 1, NFFT), device=dev)
    frames, mix = torch.empty((1, 1, 2, 2 * B), device=dev), torch.empty((1, 2, 100), device=dev)
    gains = torch.ones((1, 1), device=dev)
    st = ops._stream(x)
    n0 = lib.m2h_launch_count()
    _lib.check(lib.m2h_render_spectra(ops._ptr(x), ops._ptr(tw), ops._ptr(xspec), 1, 1, 1, 100, 0, 0, 100, 1, 0, 1, st), "spectra")
    assert ops.last_kernel() == "render_spectra"
    _lib.check(lib.m2h_render_spectra(ops._ptr(h), ops._ptr(tw), ops._ptr(hspec), 1, 1, 2, 100, 100, 1, 50, 2, 0, 1, st), "spectra")      # both ears
    _lib.check(lib.m2h_render_frames(ops._ptr(xspec), ops._ptr(hspec), ops._ptr(tw), ops._ptr(frames), 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, st), "frames")
    assert ops.last_kernel() == "render_frames"
    _lib.check(lib.m2h_render_mix(ops._ptr(frames), ops._ptr(gains), ops._ptr(mix), None, 1, 1, 0, 1, 1, 0, 1, 100, st), "mix")
    assert ops.last_kernel() == "render_mix"
    assert lib.m2h_launch_count() == n0 + 4
    assert torch.equal(mix, aur.render(x, h, gains=gains))


@pytest.mark.parametrize("L,Lr", [(16000, 16000), (900, 1000)])
def test_one_block_one_partition_against_fftconv_full(dev, aur, L, Lr):
    """J = Pn = 1: the image is m2h_fftconv_full's full[..., :L + Lr - 1] (the 32768-point transform) within twice the single-product
    bound -- each is within one of the float64 product."""
    x, h = REF.make_sources(2, 2, L, 5), REF.make_rirs(2, 2, 1, Lr, 5)[:, :, 0]
    xs, hs = _gpu(dev, x, h)
    _, images = aur.render(xs, hs, tail=True, return_images=True)
    full = torch.empty((2, 2, 2, 32768), device=dev)
    xspec = torch.empty((4, 2 * 32768), device=dev)
    _lib.check(_lib.load().m2h_fftconv_full(ops._ptr(xs), ops._ptr(hs), ops._ptr(aur._twiddle_table()), ops._ptr(xspec), ops._ptr(full), 4, L, Lr, 15,
                                            ops._stream(xs)), "m2h_fftconv_full")
    got, ref = images.cpu().numpy(), full[..., :L + Lr - 1].cpu().numpy()
    d = np.abs(got - ref).max()
    print("render vs fftconv_full L=%d Lr=%d: max-abs %.3e of bound %.3e" % (L, Lr, d, 2 * REF.PRODUCT_BOUND * np.abs(ref).max()))
    assert np.isfinite(got).all() and d <= 2 * REF.PRODUCT_BOUND * np.abs(ref).max()


def test_argument_errors_launch_nothing(dev, aur):
    from m2h.audio.render import Auralizer
    lib = _lib.load()
    x, h = _gpu(dev, REF.make_sources(2, 2, 40001, 1), REF.make_rirs(2, 2, 3, 500, 1))
    aur._twiddle_table()
    n0 = lib.m2h_launch_count()
    bad = [
        (RuntimeError, dict(sources=x.double())),                                        # dtype
        (RuntimeError, dict(rirs=h.half())),
        (RuntimeError, dict(sources=x.cpu())),                                           # device
        (RuntimeError, dict(rirs=h.cpu())),
        (ValueError, dict(sources=x[0])),                                                # rank
        (ValueError, dict(rirs=h[..., 0])),
        (ValueError, dict(rirs=h[..., :1])),                                             # one ear
        (ValueError, dict(rirs=h[:1])),                                                  # another batch
        (ValueError, dict(rirs=h[:, :, :2])),                                            # K = 2 of J = 3
        (ValueError, dict(gains=torch.ones((2, 3), device=dev))),                        # gains shape
        (ValueError, dict(gains=torch.ones((2,), device=dev))),
        (RuntimeError, dict(gains=torch.ones((2, 2), device=dev, dtype=torch.float64))),
        (ValueError, dict(sources=x[:, :, :0])),                                         # empty
        (ValueError, dict(sources=x[:, :, :16000], rirs=torch.zeros((2, 2, 256001, 2), device=dev))),   # 17 partitions
    ]
    for exc, kw in bad:
        args = dict(sources=x, rirs=h)
        args.update(kw)
        with pytest.raises(exc):
            aur.render(**args)
    with pytest.raises(ValueError, match="limit is 16 partitions"):
        aur.render(x[:, :, :16000].contiguous(), torch.zeros((2, 2, 256001, 2), device=dev))
    with pytest.raises(ValueError):
        Auralizer(dev, max_blocks=0)
    assert lib.m2h_launch_count() == n0


def _write_wav(path, rate, data):
    from scipy.io import wavfile
    wavfile.write(path, rate, data)


def test_cli_round_trip(dev, tmp_path):
    """int16 WAVs in; mix.wav and the target at most one int16 step from the rounded float64 definition; 44.1 kHz refused."""
    from scipy.io import wavfile
    r = np.random.default_rng(3)
    La, Lb, Lra, Lrb = 36001, 30000, 5000, 17000
    a = np.clip(np.round(3000 * r.standard_normal(La)), -32768, 32767).astype(np.int16)
    b = np.clip(np.round(3000 * r.standard_normal(Lb)), -32768, 32767).astype(np.int16)
    ha = np.round(32768 * 0.05 * REF.make_rirs(1, 1, 1, Lra, 8)[0, 0, 0]).astype(np.int16)
    hb = np.round(32768 * 0.05 * REF.make_rirs(1, 1, 1, Lrb, 9)[0, 0, 0]).astype(np.int16)
    paths = {k: str(tmp_path / (k + ".wav")) for k in ("a", "b", "ha", "hb", "mix", "target", "a44")}
    for k, v in (("a", a), ("b", b), ("ha", ha), ("hb", hb)):
        _write_wav(paths[k], 16000, v)
    cmd = [sys.executable, os.path.join(ROOT, "render.py"), "--source", paths["a"], "--rir", paths["ha"], "--source", paths["b"], "--rir", paths["hb"],
           "--gain", "0.6", "--gain", "0.3", "--out", paths["mix"], "--out-target", paths["target"]]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout
    x = np.zeros((1, 2, La), np.float64)
    x[0, 0], x[0, 1, :Lb] = a / 32768.0, b / 32768.0
    h = np.zeros((1, 2, 1, Lrb, 2), np.float64)
    h[0, 0, 0, :Lra], h[0, 1, 0] = ha / 32768.0, hb / 32768.0
    gains = np.array([[0.6, 0.3]], np.float32)
    want_mix, want_images = REF.render_f64(x, h, gains=gains)
    for key, want in (("mix", want_mix[0]), ("target", np.float64(gains[0, 0]) * want_images[0, 0])):
        rate, got = wavfile.read(paths[key])
        assert rate == 16000 and got.dtype == np.int16 and got.shape == (La, 2)
        want_i = np.clip(np.rint(want.T * 32768.0), -32768, 32767)
        assert np.abs(want_i).max() > 1000                                             # the comparison is about a signal
        step = np.abs(got.astype(np.int64) - want_i.astype(np.int64))
        print("render.py %s: %d of %d samples one int16 step off" % (key, int((step == 1).sum()), step.size))
        assert step.max() <= 1
    _write_wav(paths["a44"], 44100, a)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "render.py"), "--source", paths["a44"], "--rir", paths["ha"], "--out", paths["mix"]],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode != 0 and "44100 Hz" in res.stdout and "16000 Hz is required" in res.stdout


def test_rendered_mixture_goes_through_the_separator(dev, aur):
    """Plumbing only: a rendered 2.5 s mixture through Separator.separate with synthetic weights; no quality claim."""
    from m2h import synthetic
    from m2h.separate import Separator
    x, h = _gpu(dev, REF.make_sources(2, 2, 40000, 11), 0.05 * REF.make_rirs(2, 2, 1, 8000, 11)[:, :, 0])
    mix = aur.render(x, h)
    sep = Separator(synthetic.make_state_dict(synthetic.policy_shapes(), 2), dev, math=ops.MATH_FP32)
    y = sep.separate(mix, 4, use_memory=False)
    assert y.shape == (2, 40000) and bool(torch.isfinite(y).all())
