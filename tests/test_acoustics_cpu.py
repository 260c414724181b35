"""CPU: RoomAcoustics' definition (tests/acoustics_ref.py) against closed forms, the t30 margin on enveloped noise, the octave-band table,
the float32 restatement of every kernel inside the ceiling that pins tau, every mutant of a restatement outside the bound, and the
refusals of the entry points, of analyze() and of rir.py -- none of which launches anything.  (-s prints every measured figure.)

Measured here (python -m pytest tests/test_acoustics_cpu.py -s):
  restatement worst ratio   energy 4.9e-7 (Lr256000)   iacf 3.14e-7 (Lr30001.s11)   drr sums 3.29e-16 (Lr30001.s03)
  mutants, the least ratio / tau over their cases: hop_off_by_16 1.4e5, wrap_kept 8.2e3, bins_from_zero 2.2e6, past_end 47, lag_sign 1.4e5,
  other_ears_peak 7.6e12; decay mutants against 100 x DECAY_ULP_CHANGE: edc_forwards 2.9e14, first_bin_twice 8.3e6
  t30 margin on enveloped noise 0.263 (allowed 0.395)"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import acoustics_ref as R
from m2h.audio import acoustics as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()
REF = {}


def _ref(name):
    if name not in REF:
        REF[name] = R.analyze_f64(CASES[name])
    return REF[name]


def test_exponential_decay_closed_forms():
    T, Lr = 0.4, 64000
    a = 10.0 ** (-3.0 / (R.RATE * T))
    h = np.repeat((a ** np.arange(Lr, dtype=np.float64))[:, None], 2, 1)
    res = R.analyze_f64(h)
    assert res["onset"] == 0 and res["peak"].tolist() == [0, 0]
    r, nb = a ** 32, Lr // 16
    want_t = -60.0 / (R.RATE * 20.0 * math.log10(a))
    assert abs(want_t - T) < 1e-12
    # truncation at Lr: Lv[i] = 10 log10((r^i - r^nb) / (1 - r^nb)); over the bins down to -35 dB (i <= 240) it moves Lv by less than
    trunc = abs(10.0 * math.log10(1.0 - r ** (nb - 240)))
    tol = 1e-10 + trunc / 10.0 * 2            # (a level error d over a range of >= 10 dB moves the slope by at most 2 d / 10 of itself)
    for e in range(2):
        edt, t20, t30, c50 = res["params"][e, 0, :4]
        print("closed form  ear %d  edt %.15g t20 %.15g t30 %.15g (T %.15g)  c50 %.15g" % (e, edt, t20, t30, want_t, c50))
        for v in (edt, t20, t30):
            assert abs(v - want_t) <= tol * want_t
        want_c50 = 10.0 * math.log10((1.0 - a ** 1600) / (a ** 1600 - a ** (2 * Lr)))
        assert abs(c50 - want_c50) <= 1e-10 and abs(want_c50 - 10.0 * math.log10((1.0 - a ** 1600) / a ** 1600)) <= 1e-10


def test_delayed_halved_right_ear_closed_form():
    a = 10.0 ** (-3.0 / (R.RATE * 0.4))
    Lr = 8000
    h = np.zeros((Lr, 2))
    h[:, 0] = a ** np.arange(Lr)
    h[5:, 1] = 0.5 * h[:-5, 0]
    res = R.analyze_f64(h)
    assert res["onset"] == 0 and res["peak"].tolist() == [0, 5]          # the left ear's onset; the right ear's own would be 5
    sl = float((h[:R.WIN, 0] ** 2).sum())
    edge = float((h[R.WIN - 5:R.WIN, 0] ** 2).sum())                        # the right ear's window holds the left's less its last 5 samples
    want = 1.0 / math.sqrt(1.0 - edge / sl)
    print("iacc %.15g at %g, closed form %.15g" % (res["iacc"][0, 0], res["iacc"][0, 1], want))
    assert res["iacc"][0, 1] == 5 and abs(res["iacc"][0, 0] - want) <= 1e-12


@pytest.mark.parametrize("T", [0.3, 0.6, 1.2])
def test_t30_of_enveloped_noise_lies_within_the_margin(T):
    worst = 0.0
    for seed in range(100, 108):
        h = R.envelope_rir(int(1.5 * T * R.RATE), T, seed)
        n0 = R.onset_f64(h)[0]
        E = R.bins_f64(R.bands_f64(h), n0, h.shape[0])
        t30 = np.array([[R.decay_f64(E[e, b])[2] for b in range(A.BANDS)] for e in range(2)])
        worst = max(worst, float((np.abs(t30 - T) / T).max()))
    print("T %.1f  worst |t30 - T| / T %.4f (seen %.4f, margin %.4f)" % (T, worst, R.T30_WORST_SEEN, R.T30_MARGIN))
    assert worst <= R.T30_MARGIN and R.T30_MARGIN == 1.5 * R.T30_WORST_SEEN


def test_filter_table():
    m = A.octave_masks()
    assert m.shape == (6, A.NFFT) and m.dtype == np.float32
    assert np.array_equal(m[:, 1:], m[:, :0:-1])                            # real and symmetric: a zero-phase filter
    f = np.arange(A.NFFT // 2 + 1) * (R.RATE / A.NFFT)
    for b, fc in enumerate(A.BAND_CENTRES):
        db = 20.0 * np.log10(np.maximum(np.abs(m[b, :A.NFFT // 2 + 1].astype(np.float64)), 1e-30))
        at = db[int(round(fc * A.NFFT / R.RATE))]
        out = db[(f <= fc / math.sqrt(2.0) / 2.0) | (f >= fc * math.sqrt(2.0) * 2.0)]
        print("band %6g Hz  %.5f dB at fc, %.1f dB at most an octave outside the edges" % (fc, at, out.max()))
        assert abs(at) <= 0.1 and out.max() <= -60.0 and out.size > 0
    taps = A.octave_taps()
    assert taps.shape == (6, 4097) and np.array_equal(taps, taps[:, ::-1])
    import scipy.signal
    for b, fc in enumerate(A.BAND_CENTRES):                                  # the same design from scipy: ideal band-pass x Kaiser 8.6, unscaled
        want = scipy.signal.firwin(4097, [fc / math.sqrt(2.0), fc * math.sqrt(2.0)], window=("kaiser", 8.6), pass_zero=False, scale=False, fs=R.RATE)
        assert np.abs(taps[b] - want).max() <= 1e-15


def _ratios(name, got):
    ref, h = _ref(name), CASES[name]
    out = {}
    if "energy" in got:
        out["energy"] = R.ratio(got["energy"], ref["energy"], R.energy_scale(h, ref["onset"], ref["energy"]))
    if "iacf" in got:
        out["iacf"] = R.ratio(got["iacf"], ref["iacf"], R.iacf_scale(ref["iacf"]))
    if "sums" in got:
        out["drr_sums"] = R.ratio(got["sums"], ref["sums"], ref["sums"])
    return out


# which cases can show a mutant: an onset past 0, a second segment, a partial last bin with a filter tail behind it, ears that differ
_LONG = ("two_segments_lead300", "Lr30001", "Lr30001.s05", "Lr256000")
MUTANT_CASES = {"hop_off_by_16": _LONG, "wrap_kept": _LONG, "bins_from_zero": ("two_segments_lead300", "Lr30001.s05", "Lr256000"),
                "past_end": ("two_segments_lead300", "Lr30001", "Lr700"), "lag_sign": ("Lr700",) + _LONG, "other_ears_peak": ("Lr700",) + _LONG}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_fits_and_mutants_do_not(name):
    h, ref = CASES[name], _ref(name)
    got = R.analyze_fp32(h)
    assert got["onset"] == ref["onset"] and got["peak"].tolist() == ref["peak"].tolist()
    for k, v in _ratios(name, got).items():
        print("restatement  %-22s %-9s %.3e of ceiling %.3e (tau %.3e)" % (name, k, v, R.RESTATEMENT_WORST[k], R.TAU[k]))
        assert v <= R.RESTATEMENT_WORST[k]
    dev = R.param_dev(got["params"], ref["params"])
    assert np.array_equal(np.isnan(got["iacc"]), np.isnan(ref["iacc"]))
    di = float(np.max(np.nan_to_num(np.abs(got["iacc"] - ref["iacc"])[..., 0])))
    print("end to end   %-22s %s  iacc %.2e" % (name, " ".join("%s %.2e" % kv for kv in zip(A.ACOUSTIC_ORDER, dev)), di))
    assert all(d <= R.E2E_WORST[k] for k, d in zip(A.ACOUSTIC_ORDER, dev)) and di <= R.E2E_WORST["iacc"]
    assert np.array_equal(got["iacc"][..., 1], ref["iacc"][..., 1], equal_nan=True)
    for m, names in MUTANT_CASES.items():
        if name not in names:
            continue
        if m in R.ENERGY_MUTANTS:
            key, g = "energy", {"energy": R.band_energy_fp32(h, ref["onset"], m)[0]}
        elif m in R.IACF_MUTANTS:
            key, g = "iacf", {"iacf": R.band_energy_fp32(h, ref["onset"], m)[1]}
        else:
            key, g = "drr_sums", {"sums": R.onset_fp32(h, m)[2]}
        v = _ratios(name, g)[key]
        print("mutant       %-22s %-16s %.1e tau" % (name, m, v / R.TAU[key]))
        assert v > R.TAU[key]


def test_taus_are_the_stated_ones():
    assert R.TAU == {k: 8 * v for k, v in R.RESTATEMENT_WORST.items()} and set(R.TAU) == {"energy", "iacf", "drr_sums"}
    assert set(MUTANT_CASES) == set(R.ENERGY_MUTANTS + R.IACF_MUTANTS + R.DRR_MUTANTS) and all(set(v) <= set(CASES) for v in MUTANT_CASES.values())
    assert set(R.E2E_WORST) == set(A.ACOUSTIC_ORDER) | {"iacc"}
    src = open(os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc", "rir_acoustics.hip")).read()
    for text in ("constexpr int RIR_SEG_BINS = %d;" % R.SEG_BINS, "constexpr int RIR_HALF = %d;" % R.HALF, "constexpr int RIR_WIN = %d;" % R.WIN,
                 "constexpr int RIR_MAXLAG = %d;" % R.MAXLAG, "constexpr int RIR_DIRECT = %d;" % R.DIRECT, "constexpr int RIR_BIN = %d;" % R.BIN):
        assert text in src, text
    assert (R.LEAD, R.HOP, R.NFFT - 2 * R.HALF) == (2064, 12256, R.HOP + 32)


@pytest.mark.parametrize("name", sorted(R.decay_cases()))
def test_decay_algebra_one_ulp_change_and_mutants(name):
    E = R.decay_cases()[name]
    base = R.decay_f64(E)
    g = np.random.default_rng(5)
    worst = np.zeros(7)
    for _ in range(8):
        worst = np.maximum(worst, R.param_dev(R.decay_f64(E * (1.0 + np.finfo(np.float64).eps * g.choice([-1, 0, 1], E.shape))), base))
    print("decay  %-16s %s  one-ulp change %.2e (pinned %.2e)" % (name, np.array2string(base, precision=5), worst.max(), R.DECAY_ULP_CHANGE))
    assert worst.max() <= R.DECAY_ULP_CHANGE
    if np.isfinite(base[:3]).all():
        for m in R.DECAY_MUTANTS:
            dev = R.param_dev(R.decay_f64(E, m), base)
            print("mutant %-16s %-16s %.1e bounds" % (name, m, dev[:3].max() / (100 * R.DECAY_ULP_CHANGE)))
            assert dev[:3].max() > 100 * R.DECAY_ULP_CHANGE
    if name == "exp.nb1":
        assert np.isnan(base[:3]).all() and base[3] == np.inf and base[5] == 1.0 and base[6] == 0.0005
    if name == "zeros.nb100":
        assert np.isnan(base).all()


def test_silent_rir_and_silent_ear_in_the_definition():
    h = R.noise_rir(700, 0.05, 7)
    h[:, 1] = 0.0
    res = R.analyze_f64(h)
    assert res["onset"] == 0 and res["peak"].tolist() == [0, 0] and np.isnan(res["drr"][1]) and np.isfinite(res["drr"][0])
    assert np.isnan(res["params"][1]).all() and np.isfinite(res["params"][0, :, 5:]).all() and np.isnan(res["iacc"]).all()
    res = R.analyze_f64(np.zeros((700, 2), dtype=np.float32))
    assert res["onset"] == 0 and np.isnan(res["drr"]).all() and np.isnan(res["params"]).all() and np.isnan(res["iacc"]).all()


def test_entry_points_refuse_without_a_launch():
    from m2h import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)          # never dereferenced
    n0 = lib.m2h_launch_count()

    def onset(rirs=p, onset=p, peak=p, sums=p, drr=p, Q=2, Lr=100):
        return lib.m2h_rir_onset(rirs, onset, peak, sums, drr, Q, Lr, None)

    def band(rirs=p, onset=p, sums=p, masks=p, tw=p, energy=p, iacf=p, iacc=p, Q=2, Lr=100):
        return lib.m2h_rir_band_energy(rirs, onset, sums, masks, tw, energy, iacf, iacc, Q, Lr, None)

    def decay(bins=p, params=p, rows=2, nb=100):
        return lib.m2h_rir_decay(bins, params, rows, nb, None)

    rows = [(b"rir_onset", onset, [(dict(rirs=None), b"null pointer"), (dict(drr=None), b"null pointer"), (dict(Lr=0), b"Lr = 0"),
                                  (dict(Lr=256001), b"Lr = 256001"), (dict(Q=0), b"Q = 0"), (dict(sums=odd), b"8-byte aligned")]),
            (b"rir_band_energy", band, [(dict(onset=None), b"null pointer"), (dict(sums=None), b"null pointer"), (dict(masks=None), b"null pointer"), (dict(iacc=None), b"null pointer"),
                                        (dict(Lr=0), b"Lr = 0"), (dict(Lr=256001), b"Lr = 256001"), (dict(Q=0), b"Q = 0"),
                                        (dict(Q=65536), b"exceed the grid"), (dict(energy=odd), b"8-byte aligned")]),
            (b"rir_decay", decay, [(dict(bins=None), b"null pointer"), (dict(params=None), b"null pointer"), (dict(nb=0), b"nb = 0"),
                                   (dict(nb=16001), b"nb = 16001"), (dict(rows=0), b"rows = 0"), (dict(rows=1 << 34), b"rows = 17179869184"),
                                   (dict(bins=odd), b"8-byte aligned")])]
    for name, call, cases in rows:
        for kw, text in cases:
            assert call(**kw) < 0, (name, kw)
            msg = lib.m2h_last_error()
            assert msg.startswith(name + b": ") and text in msg, (name, kw, msg)
    assert lib.m2h_launch_count() == n0


def test_analyze_refuses_bad_arguments_before_any_launch():
    import torch
    from m2h import _lib
    ra = A.RoomAcoustics(torch.device("cuda", 0))
    n0 = _lib.load().m2h_launch_count()
    for bad, exc, text in ((np.zeros((4, 2), np.float32), TypeError, "torch tensor"),
                           (torch.zeros(4, 2, dtype=torch.float64), RuntimeError, "float32"),
                           (torch.zeros(4, 3), ValueError, "[..., Lr, 2]"),
                           (torch.zeros(2), ValueError, "[..., Lr, 2]"),
                           (torch.zeros(A.MAX_TAPS + 1, 2), ValueError, "256001 taps"),
                           (torch.zeros(0, 4, 2), ValueError, "hold no RIR"),
                           (torch.zeros(4, 2), RuntimeError, "must live on cuda:0")):
        with pytest.raises(exc) as e:
            ra.analyze(bad)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(RuntimeError):
        A.RoomAcoustics("cpu")
    assert _lib.load().m2h_launch_count() == n0 and A.ACOUSTIC_ORDER == ("edt", "t20", "t30", "c50", "c80", "d50", "ts")


def test_rir_cli_refuses_other_rates_and_mono_files(tmp_path):
    from scipy.io import wavfile
    g = np.random.default_rng(3)
    stereo, mono = (g.standard_normal((800, 2)) * 0.1).astype(np.float32), (g.standard_normal(800) * 0.1).astype(np.float32)
    wavfile.write(str(tmp_path / "r441.wav"), 44100, stereo)
    wavfile.write(str(tmp_path / "mono.wav"), 16000, mono)
    for name, texts in (("r441.wav", ("44100 Hz", "16000 Hz")), ("mono.wav", ("1 channel", "2 (left and right ear)"))):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "rir.py"), "--rir", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode != 0 and all(t in r.stdout for t in texts) and "rir.py: " in r.stdout, r.stdout
