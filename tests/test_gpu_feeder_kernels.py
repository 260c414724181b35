"""GPU: the audio feeder and the evaluation inverse transform -- csrc/stft.hip (stft_frames, stft_post, istft_pre, istft_ola,
feeder_round_mix, rms_normalize, bss_metrics), csrc/fftconv.hip (all five instances) and the two DFT-as-GEMM calls of m2h/audio/stft.py -- on
every row of tests/feeder_kernels.py's table through the entry point the project itself uses (ops.linear, ops.bss_metrics,
BinauralFeeder.convolve_round, and the library calls as m2h/audio/stft.py and feeder.py make them), every output element against the float64
reference of the same float32 inputs: |g_e - r_e| <= tau * s_e (the scales, the two tie rules and the taus: tests/feeder_kernels.py, pinned
on the CPU by tests/test_feeder_kernels_cpu.py together with the mutants the bound must reject).  Every output buffer is prefilled with a
sentinel and the scratch of the convolution with NaN; what a kernel must not write keeps the sentinel, what it must not read is NaN (or a
poison value where a NaN would turn into a plausible number).

Worst |g - r| / s measured on an MI355X over each family's rows (test_zz_report_worst_ratios prints them with -s), and the tau it is held to:
  frames     exact
  dft        stft 1.29e-6, istft 1.15e-6                                                   TAU_FP32 = 2e-5
  post       mode 0: |X| 1.10e-7, phase 1.91e-7; mode 1: log1p 7.4e-8, phase 1.96e-7; mode 2: 5.9e-8, every fp16 value exact outside
             tie rule 1 (at most 0.196 % of a row left out)                                 TAU_FP32
  pre        1.04e-7 (phases to 8 pi: 9.95e-8); columns [2 nb, ldr) keep the sentinel     TAU_FP32
  ola        1.28e-7; zero fill and the undivided zeros exact                             TAU_FP32
  round_mix  exact
  rms        1.65e-7                                                                      TAU_FP32
  bss        clips 5.3e-8, DC-heavy 2.5e-8, near-perfect 4.1e-8 (of a bound of 0.6e-3 .. 5e-2 dB)   TAU_FP32
  fftconv    feeder kind 1.52e-6, DC-heavy 8.2e-7 (tau 1.3e-5); impulse rows 3.90e-5 (their own tau 3.2e-4) -- the float32 numpy restatement's
             figures to two digits, all five instances
  chain      near-tie shares 0.83 % and 0.93 %, samples one LSB off 0.0094 % and 0.0061 %, none outside tie rule 2; mixtures exact
The 286 tests of this file take 7 s on an MI355X; no row found a kernel defect.
"""
import numpy as np
import pytest
import torch

import feeder_kernels as Fk
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
WORST = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) if a is not None else None


def _full(shape, value):
    return torch.full(shape, value, dtype=torch.float32, device=_dev())


def _ids(family, pred=lambda r: True):
    return [r["id"] for r in Fk.ROWS[family] if pred(r)]


def _call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _check_row(row, got, ref, kind=None):
    """Every output of the row against (r, s[, skip]); one printed line per row: worst ratio, scale - 1, the share left out."""
    family, tau = row["family"], Fk.tau_of(row)
    line_w, line_s, fails, left = 0.0, 0.0, [], 0.0
    for name, rs in ref.items():
        r, s = rs[0], rs[1]
        skip = rs[2] if len(rs) > 2 else None
        g = got[name].detach().cpu().numpy()
        assert g.size == np.size(r), (row["id"], name, g.shape, np.shape(r))
        worst, scale, ok = Fk.check(g, r, s, tau, skip)
        key = (family, kind or row.get("kind", ""), name)
        WORST[key] = max(WORST.get(key, 0.0), worst)
        line_w = max(line_w, worst)
        line_s = scale - 1.0 if abs(scale - 1.0) > abs(line_s) else line_s
        left = max(left, float(np.mean(skip)) if skip is not None else 0.0)
        if not ok:
            fails.append((name, worst, scale))
    print("%-62s worst |g-r|/s %.2e  scale-1 %+.1e  left out %.3f %%" % (row["id"], line_w, line_s, 100 * left))
    assert not fails, (row["id"], fails)


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", _ids("frames"))
def test_stft_frames_are_the_exact_windowed_reflection(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    y, w = _d(inp["y"]), _d(inp["window"])
    S, L, T, n_fft, hop, ldf = (row[k] for k in ("S", "L", "T", "n_fft", "hop", "ldf"))
    frames = _full((S, T, ldf), Fk.SENT)
    _call("m2h_stft_frames", ops._ptr(y), ops._ptr(w), ops._ptr(frames), S, L, T, n_fft, hop, ldf, ops._stream(y))
    assert ops.last_kernel() == "stft_frames"
    torch.cuda.synchronize()
    _check_row(row, dict(frames=frames), Fk.reference(row, inp))


@pytest.mark.parametrize("row_id", _ids("dft"))
def test_dft_as_gemm_matches_fp64(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    from m2h.audio.stft import ISTFT, STFT
    t = STFT(_dev()) if row["which"] == "stft" else ISTFT(_dev())
    assert np.array_equal(t.W.cpu().numpy(), inp["W"])         # the matrix the class built on the device's side is the one referenced
    y = ops.linear(_d(inp["x"]), t.W, None, name="stft.dft" if row["which"] == "stft" else "istft.idft")
    torch.cuda.synchronize()
    _check_row(row, dict(y=y), Fk.reference(row, inp), kind=row["which"])


@pytest.mark.parametrize("row_id", _ids("post"))
def test_stft_post_matches_fp64(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    B, C, T, nb, lds = (row[k] for k in ("B", "C", "T", "nb", "lds"))
    spec = _d(inp["spec"])
    mag = _full((B, nb, T, C), Fk.SENT) if row["outs"] != "phase" else None
    phase = _full((B, nb, T, C), Fk.SENT) if row["outs"] != "mag" else None
    _call("m2h_stft_post", ops._ptr(spec), ops._ptr(mag), ops._ptr(phase), B, C, T, nb, lds, row["mode"], ops._stream(spec))
    assert ops.last_kernel() == "stft_post"
    torch.cuda.synchronize()
    got = {k: v for k, v in (("mag", mag), ("phase", phase)) if v is not None}
    ref = Fk.reference(row, inp)
    assert set(got) == set(ref)
    n = len(Fk.POST_PLANTS)
    if mag is not None:
        g = mag.cpu().numpy()[0, :n, 0, 0]
        assert (g[:4] == 0).all(), g[:4]                       # the planted zeros: exact
        if row["mode"] == 2:
            assert np.isinf(g[13]) and g[13] > 0 and g[14] == np.float32(np.log1p(65504.0))       # above 65520: inf, as astype(float16)
    if phase is not None:      # signed zeros and the negative real axis, as numpy's arctan2
        g = phase.cpu().numpy()[0, :n, 0, 0]
        assert g[0] == 0 and not np.signbit(g[0]) and g[2] == 0 and np.signbit(g[2])
        assert np.array_equal(g[[1, 3, 7, 8, 4]], np.array([np.pi, -np.pi, np.pi, -np.pi, np.pi / 2], dtype=np.float32)), g[:n]
    _check_row(row, got, ref, kind="mode %d" % row["mode"])


@pytest.mark.parametrize("row_id", _ids("pre"))
def test_istft_pre_matches_fp64(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    B, T, nb, ldr, C, c = (row[k] for k in ("B", "T", "nb", "ldr", "C", "c"))
    mag, phase = _d(inp["mag"]), _d(inp["phase"])
    rows = _full((B, T, ldr), Fk.SENT)
    _call("m2h_istft_pre", ops._ptr(mag), ops._ptr(phase), ops._ptr(rows), B, C, c, T, nb, ldr, ops._stream(mag))
    assert ops.last_kernel() == "istft_pre"
    torch.cuda.synchronize()
    assert bool((rows[..., 2 * nb:] == Fk.SENT).all())          # columns [2 nb, ldr) are not the kernel's to write
    _check_row(row, dict(rows=rows), Fk.reference(row, inp), kind="wide" if row["wide"] else "")


@pytest.mark.parametrize("row_id", _ids("ola"))
def test_istft_ola_matches_fp64(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    S, T, n_fft, hop, ldf, length = (row[k] for k in ("S", "T", "n_fft", "hop", "ldf", "length"))
    fr, w = _d(inp["frames"]), _d(inp["window"])
    y = _full((S, length), Fk.SENT)
    _call("m2h_istft_ola", ops._ptr(fr), ops._ptr(w), ops._ptr(y), S, T, n_fft, hop, ldf, length, ops._stream(fr))
    assert ops.last_kernel() == "istft_ola"
    torch.cuda.synchronize()
    _check_row(row, dict(y=y), Fk.reference(row, inp))


@pytest.mark.parametrize("row_id", _ids("round_mix"))
def test_feeder_round_mix_is_exact(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    S, L = row["S"], row["L"]
    full, mix = _d(inp["full"]), _d(inp["mix"])
    conv = _full((S, L), Fk.SENT) if row["conv"] else None
    _call("m2h_feeder_round_mix", ops._ptr(full), row["ldfull"], row["start"], ops._ptr(conv), ops._ptr(mix), S, L, row["first"], row["scale"], ops._stream(full))
    assert ops.last_kernel() == "feeder_round_mix"
    torch.cuda.synchronize()
    ref = Fk.reference(row, inp)
    if conv is None:
        del ref["conv_out"]
    _check_row(row, dict(conv_out=conv, mix=mix), ref)


@pytest.mark.parametrize("row_id", _ids("rms"))
def test_rms_normalize_matches_fp64(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    mag = _d(inp["mag"])
    _call("m2h_rms_normalize", ops._ptr(mag), row["S"], row["n"], Fk.RMS_NORM, ops._stream(mag))
    assert ops.last_kernel() == "rms_normalize"
    torch.cuda.synchronize()
    if row["zero"]:
        assert bool((mag[1] == 0).all()) and bool(torch.isfinite(mag).all())
    _check_row(row, dict(mag=mag), Fk.reference(row, inp))


@pytest.mark.parametrize("row_id", _ids("bss"))
def test_bss_metrics_match_fp64(row_id):
    """The well-conditioned outputs in dB against the function-of-sums scale; si_sir, si_sar and their improvements divide by rounding
    noise, in the reference as here: finite, and si_sir > 60 dB (tests/test_gpu_eval_metrics.py's assertions)."""
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    out = ops.bss_metrics(_d(inp["ref"]), _d(inp["est"]), _d(inp["mix_l"]), _d(inp["mix_r"]))
    assert ops.last_kernel() == "bss_metrics" and out.shape == (row["S"], Fk.N_METRICS)
    torch.cuda.synchronize()
    if row["L"] > 2:
        g = out.cpu().numpy()
        assert np.isfinite(g).all() and bool((g[:, 1] > 60).all()), g
    _check_row(row, dict(out=out), Fk.reference(row, inp))


def _run_fftconv(row, inp):
    CS, L, Lr, n = row["CS"], row["L"], row["Lr"], row["log2n"]
    nfft = 1 << n
    from m2h.audio.feeder import BinauralFeeder
    tw = BinauralFeeder(_dev())._twiddle_table(nfft)
    assert np.array_equal(tw.cpu().numpy(), inp["tw"])
    mono, rirs = _d(inp["mono"]), _d(inp["rirs"])
    full = _full((CS, 2, nfft), Fk.SENT)
    xspec = _full((CS, 2 * nfft), float("nan"))
    _call("m2h_fftconv_full", ops._ptr(mono), ops._ptr(rirs), ops._ptr(tw), ops._ptr(xspec), ops._ptr(full), CS, L, Lr, n, ops._stream(mono))
    assert ops.last_kernel() == "fftconv_same"
    torch.cuda.synchronize()
    return full


@pytest.mark.parametrize("row_id", _ids("fftconv"))
def test_fftconv_full_matches_fp64_convolution(row_id):
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    _check_row(row, dict(full=_run_fftconv(row, inp)), Fk.reference(row, inp))


@pytest.mark.parametrize("row_id", _ids("chain"))
def test_convolve_round_rounds_like_fp64_but_near_ties(row_id):
    """Tie rule 2: a per-source sample equals round(float64 convolution), wrapped and scaled, but where the float64 value lies within
    tau s of a half-integer -- there one LSB; the mixture is exact from the per-source values the kernels made."""
    from m2h.audio.feeder import BinauralFeeder
    row = Fk.ROWS_BY_ID[row_id]
    inp = Fk.inputs(row)
    per, mix = BinauralFeeder(_dev()).convolve_round(_d(inp["mono"]), _d(inp["rirs"]))
    torch.cuda.synchronize()
    q, near = Fk.chain_reference(row, inp)["per_source"]
    share = float(near.mean())
    assert share <= Fk.TIE2_CAP
    got = [p.cpu().numpy() for p in per]
    g = np.stack(got).astype(np.float64) * 32768
    flips = float((g != q).mean())
    print("%-62s near-tie share %.3f %%, flips %.4f %%, flips outside the rule %d" % (row_id, 100 * share, 100 * flips, int((g != q)[~near].sum())))
    WORST[("chain", "", "flips %")] = max(WORST.get(("chain", "", "flips %"), 0.0), 100 * flips)
    assert np.array_equal(g[~near], q[~near]) and float(np.abs(g - q).max()) <= 1.0
    assert np.array_equal(mix.cpu().numpy(), Fk.chain_mix(got))


def test_zz_report_worst_ratios():
    """(summary, with -s: the worst ratio per family, kind and output over the rows that ran -- the figures of the module docstring)"""
    for key, v in sorted(WORST.items()):
        print("worst  %-10s %-14s %-10s %.2e" % (key + (v,)))
