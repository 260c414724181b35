"""RoomAcoustics in float64 numpy / scipy (the definition of m2h/audio/acoustics.py, restated), a float32 restatement of each kernel of
csrc/rir_acoustics.hip with the kernel's own segmenting (the transforms through scipy.fft in single precision), the mutants of those
restatements, the scales of the element bounds and the cases the CPU and the GPU test share.

Bounds, by the project's rule |g - r| <= tau . s:
  energy bin   s = ||z_segment||^2 / 16384 + E      z_segment: the 16384 complex samples the bin's segment transforms
  IACF sum     s = sqrt(sum_W y_L^2 . sum_W y_R^2)   (the two energies that stand beside the 33 lag sums: their own value)
  drr sums     s = the sum itself (fp64, exact products: tau is for the order of summation only)
tau = 8 x RESTATEMENT_WORST, the worst ratio of the float32 restatement over CASES, measured on the CPU (test_acoustics_cpu.py pins it)."""
import numpy as np
import scipy.fft
import scipy.signal

from m2h.audio import acoustics as A

RATE, BIN, NFFT, HALF = 16000, 16, 16384, 2048
LEAD, SEG_BINS = HALF + 16, 766
HOP = SEG_BINS * BIN
WIN, MAXLAG, DIRECT = 1280, 16, 40
RANGES = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))
NAN = float("nan")

# worst |restatement - reference| / scale over CASES, measured on the CPU, rounded up; the GPU is held to 8 x
RESTATEMENT_WORST = {"energy": 5.0e-7, "iacf": 3.2e-7, "drr_sums": 3.3e-16}
TAU = {k: 8 * v for k, v in RESTATEMENT_WORST.items()}
# end to end (test_gpu_acoustics.py): worst deviation of the composed float32 restatement from the definition on the noise RIRs, per parameter
# (relative for the times, d50 and ts; absolute dB for c50, c80; absolute for the IACC value); the GPU is held to 8 x
E2E_WORST = {"edt": 7.8e-8, "t20": 1.8e-7, "t30": 1.9e-7, "c50": 8.9e-7, "c80": 1.5e-6, "d50": 1.2e-7, "ts": 6.3e-8, "iacc": 9.3e-8}
# m2h_rir_decay on bins of the test's making: the largest change of the float64 algebra under a one-ulp relative perturbation of the bins
# (relative for the times, d50, ts; absolute dB for c50, c80), measured on DECAY_CASES on the CPU; the GPU is held to 100 x
DECAY_ULP_CHANGE = 3.6e-15
# noise under a 60 dB exponential envelope of T = 0.3, 0.6, 1.2 s (envelope_rir, 1.5 T long, seeds 100 .. 107): the worst |t30 - T| / T of the
# float64 definition over every band and ear is 0.263 (the 125 Hz octave, 88 Hz wide); the test allows 1.5 x
T30_WORST_SEEN = 0.2635
T30_MARGIN = 1.5 * T30_WORST_SEEN

_TAPS = A.octave_taps()
_MASKS = A.octave_masks()


# ---------------------------------------------------------------- the definition, float64

def onset_f64(h):
    """h [Lr, 2] -> n0, npk [2], (D, T) [2, 2], drr [2]"""
    h = np.asarray(h, dtype=np.float64)
    Lr = h.shape[0]
    mag = np.abs(h)
    pk = mag.max(0)
    npk = [int(np.argmax(mag[:, e])) if pk[e] > 0 else 0 for e in range(2)]
    firsts = [int(np.argmax(mag[:, e] >= 0.1 * pk[e])) for e in range(2) if pk[e] > 0]
    n0 = min(firsts) if firsts else 0
    sums, drr = np.zeros((2, 2)), np.full(2, NAN)
    for e in range(2):
        lo, hi = max(0, npk[e] - DIRECT), min(Lr, npk[e] + DIRECT + 1)
        D, T = float((h[lo:hi, e] ** 2).sum()), float((h[:, e] ** 2).sum())
        sums[e] = D, T
        if pk[e] > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                drr[e] = 10.0 * np.log10(np.float64(D) / np.float64(T - D))
    return n0, npk, sums, drr


def bands_f64(h):
    """h [Lr, 2] -> y [7, Lr + 2 HALF, 2]: y[b, HALF + n] is band b at sample n, n = -HALF .. Lr + HALF - 1"""
    h = np.asarray(h, dtype=np.float64)
    Lr = h.shape[0]
    y = np.zeros((A.BANDS, Lr + 2 * HALF, 2))
    y[0, HALF:HALF + Lr] = h
    for b in range(1, A.BANDS):
        for e in range(2):
            y[b, :, e] = scipy.signal.fftconvolve(h[:, e], _TAPS[b - 1])
    return y


def bins_f64(y, n0, Lr):
    """-> E [2, 7, ceil(Lr / 16)] (zeros past Nb)"""
    nbs = -(-Lr // BIN)
    E = np.zeros((2, A.BANDS, nbs))
    seg = y[:, HALF + n0:HALF + Lr] ** 2
    pad = (-seg.shape[1]) % BIN
    seg = np.concatenate([seg, np.zeros((A.BANDS, pad, 2))], 1).reshape(A.BANDS, -1, BIN, 2).sum(2)
    E[:, :, :seg.shape[1]] = seg.transpose(2, 0, 1)
    return E


def iacf_f64(y, n0):
    """-> sums [7, 35]: k < 33 the lag k - 16, 33 sum L^2, 34 sum R^2"""
    out = np.zeros((A.BANDS, 2 * MAXLAG + 3))
    t = HALF + n0 + np.arange(WIN)
    for b in range(A.BANDS):
        L = y[b, t, 0]
        for k in range(2 * MAXLAG + 1):
            out[b, k] = float((L * y[b, t + k - MAXLAG, 1]).sum())
        out[b, 33], out[b, 34] = float((L * L).sum()), float((y[b, t, 1] ** 2).sum())
    return out


def iacc_of(sums):
    """sums [..., 35] -> [..., 2]: (max |IACF|, lag), the lowest lag on ties"""
    sums = np.asarray(sums, dtype=np.float64)
    out = np.full(sums.shape[:-1] + (2,), NAN)
    den = np.sqrt(sums[..., 33] * sums[..., 34])
    for ix in np.ndindex(sums.shape[:-1]):
        if den[ix] > 0:
            v = np.abs(sums[ix][:2 * MAXLAG + 1]) / den[ix]
            k = int(np.argmax(v))
            out[ix] = v[k], k - MAXLAG
    return out


def decay_f64(E, mutant=None):
    """E [nb] -> the 7 parameters in ACOUSTIC_ORDER"""
    E = np.asarray(E, dtype=np.float64)
    nb = E.shape[0]
    edc = np.cumsum(E[::-1])[::-1] if mutant != "edc_forwards" else np.cumsum(E)
    out = np.full(7, NAN)
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = 10.0 * np.log10(edc / edc[0]) if mutant != "edc_forwards" else 10.0 * np.log10(edc / edc[-1])
        t = np.arange(nb) / 1000.0
        for r, (lo, hi) in enumerate(RANGES):
            idx = np.nonzero((lv <= lo) & (lv >= hi))[0]
            if mutant == "first_bin_twice" and lo == -5.0 and idx.size:
                idx = np.concatenate([idx[:1], idx])
            if idx.size >= 2:
                x, v = t[idx] - t[idx].mean(), lv[idx] - lv[idx].mean()
                out[r] = -60.0 / ((x * v).sum() / (x * x).sum())
        tot = E.sum()
        for j, k in ((3, 50), (4, 80)):
            out[j] = 10.0 * np.log10(E[:k].sum() / E[k:].sum())
        out[5] = E[:50].sum() / tot
        out[6] = ((np.arange(nb) + 0.5) / 1000.0 * E).sum() / tot
    return out


def analyze_f64(h):
    """h [Lr, 2] fp32 -> dict of the definition's results for one RIR"""
    Lr = h.shape[0]
    n0, npk, sums, drr = onset_f64(h)
    y = bands_f64(h)
    E = bins_f64(y, n0, Lr)
    iacf = iacf_f64(y, n0)
    params = np.array([[decay_f64(E[e, b]) for b in range(A.BANDS)] for e in range(2)])
    return {"onset": n0, "peak": np.array(npk), "sums": sums, "drr": drr, "energy": E, "iacf": iacf, "iacc": iacc_of(iacf), "params": params}


# ---------------------------------------------------------------- scales

def segment_norms(h, n0):
    """||z_segment||^2 for every segment g of the kernel's grid"""
    h = np.asarray(h, dtype=np.float64)
    Lr = h.shape[0]
    segs = -(-(-(-Lr // BIN)) // SEG_BINS)
    out = np.zeros(segs)
    for g in range(segs):
        a = n0 - LEAD + HOP * g
        out[g] = float((h[max(a, 0):max(min(a + NFFT, Lr), 0)] ** 2).sum())
    return out


def energy_scale(h, n0, E):
    nbs = E.shape[-1]
    z = np.repeat(segment_norms(h, n0), SEG_BINS)[:nbs] / NFFT
    return z[None, None, :] + E


def iacf_scale(iacf):
    """sqrt(sum L^2 . sum R^2) for the 33 lag sums; the two energies by their own value"""
    s = np.repeat(np.sqrt(iacf[..., 33] * iacf[..., 34])[..., None], iacf.shape[-1], -1)
    s[..., 33:] = iacf[..., 33:]
    return s


def ratio(g, r, s):
    """worst |g - r| / s; inf where s = 0 and g != r, or where NaN and number disagree"""
    g, r, s = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (g, r, s))
    if (np.isnan(g) != np.isnan(r)).any():
        return float("inf")
    ok = ~np.isnan(r)
    d = np.abs(g[ok] - r[ok])
    s = s[ok]
    if ((s == 0) & (d > 0)).any():
        return float("inf")
    nz = s > 0
    return float((d[nz] / s[nz]).max()) if nz.any() else 0.0


def param_dev(g, r):
    """worst deviation of parameter rows [..., 7]: relative for edt, t20, t30, d50, ts, absolute (dB) for c50, c80; NaN and inf must agree"""
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    out = np.zeros(7)
    for j in range(7):
        a, b = g[..., j].reshape(-1), r[..., j].reshape(-1)
        if (np.isnan(a) != np.isnan(b)).any() or (np.isinf(a) != np.isinf(b)).any() or (a[np.isinf(b)] != b[np.isinf(b)]).any():
            out[j] = float("inf")
            continue
        ok = np.isfinite(b)
        if ok.any():
            d = np.abs(a[ok] - b[ok])
            out[j] = float((d if j in (3, 4) else d / np.where(b[ok] == 0, 1.0, np.abs(b[ok]))).max())       # (absolute where the reference is 0)
    return out


# ---------------------------------------------------------------- the kernels, restated in float32

def onset_fp32(h, mutant=None):
    """m2h_rir_onset: 1024 threads at stride 1024, then a pairwise tree"""
    h32 = np.asarray(h, dtype=np.float32)
    n0, npk, _, _ = onset_f64(h32)
    Lr = h32.shape[0]
    sums = np.zeros((2, 2))
    for e in range(2):
        c = npk[1 - e] if mutant == "other_ears_peak" else npk[e]
        sq = h32[:, e].astype(np.float64) ** 2
        inside = (np.arange(Lr) >= c - DIRECT) & (np.arange(Lr) <= c + DIRECT)
        for j, v in enumerate((np.where(inside, sq, 0.0), sq)):
            part = np.zeros(1024)
            for k in range(0, Lr, 1024):
                part[:min(1024, Lr - k)] += v[k:k + 1024]
            while part.size > 1:
                part = part[:part.size // 2] + part[part.size // 2:]
            sums[e, j] = part[0]
    return n0, npk, sums


def band_energy_fp32(h, n0, mutant=None):
    """m2h_rir_band_energy: -> E [2, 7, nbs], iacf [7, 35]"""
    h32 = np.asarray(h, dtype=np.float32)
    Lr = h32.shape[0]
    nbs = -(-Lr // BIN)
    segs = -(-nbs // SEG_BINS)
    start = 0 if mutant == "bins_from_zero" else n0
    hop = HOP + 16 if mutant == "hop_off_by_16" else HOP
    lead = 16 if mutant == "wrap_kept" else LEAD
    E, iacf = np.zeros((2, A.BANDS, nbs)), np.zeros((A.BANDS, 2 * MAXLAG + 3))
    live = [bool(np.any(h32[:, e] != 0)) for e in range(2)]             # a silent ear stays silent: the shared transform's rounding is not let into it
    for g in range(segs):
        a = start - lead + hop * g
        if start + HOP * g >= Lr and g > 0:
            continue
        z = np.zeros(NFFT, dtype=np.complex64)
        lo, hi = max(a, 0), min(a + NFFT, Lr)
        if hi > lo:
            z[lo - a:hi - a] = h32[lo:hi, 0] + 1j * h32[lo:hi, 1]
        Z = None
        for b in range(A.BANDS):
            if b == 0:
                y = z
            else:
                if Z is None:
                    Z = scipy.fft.fft(z)
                y = scipy.fft.ifft((Z * _MASKS[b - 1]).astype(np.complex64))
            assert y.dtype == np.complex64
            y = (y.real if live[0] else 0 * y.real) + 1j * (y.imag if live[1] else 0 * y.imag)
            n = a + lead + np.arange(HOP)
            keep = n < (Lr + BIN if mutant == "past_end" else Lr)
            for e, part in enumerate((y.real, y.imag)):
                v = np.where(keep, part[lead:lead + HOP].astype(np.float64), 0.0) ** 2
                bins = v.reshape(SEG_BINS, BIN).sum(1)
                m = min(SEG_BINS, nbs - SEG_BINS * g)
                E[e, b, SEG_BINS * g:SEG_BINS * g + m] = bins[:m]
            if g == 0:
                t = lead + np.arange(WIN)
                L, R = y.real.astype(np.float64), y.imag.astype(np.float64)
                sign = -1 if mutant == "lag_sign" else 1
                for k in range(2 * MAXLAG + 1):
                    iacf[b, k] = (L[t] * R[t + sign * (k - MAXLAG)]).sum()
                iacf[b, 33], iacf[b, 34] = (L[t] ** 2).sum(), (R[t] ** 2).sum()
    return E, iacf


def analyze_fp32(h):
    """the three kernels composed (the decay algebra is fp64 on the device as in decay_f64)"""
    n0, npk, sums = onset_fp32(h)
    E, iacf = band_energy_fp32(h, n0)
    params = np.array([[decay_f64(E[e, b]) for b in range(A.BANDS)] for e in range(2)])
    return {"onset": n0, "peak": np.array(npk), "sums": sums, "energy": E, "iacf": iacf, "iacc": iacc_of(iacf), "params": params}


ENERGY_MUTANTS = ("hop_off_by_16", "wrap_kept", "bins_from_zero", "past_end")
IACF_MUTANTS = ("lag_sign",)
DRR_MUTANTS = ("other_ears_peak",)
DECAY_MUTANTS = ("edc_forwards", "first_bin_twice")


# ---------------------------------------------------------------- cases

def noise_rir(Lr, T60, seed, lead=0, delay=5, right_gain=0.7):
    """Noise under a 60 dB exponential envelope, a direct impulse in front; the right ear later and weaker; `lead` silent samples first."""
    g = np.random.default_rng(seed)
    n = np.arange(Lr, dtype=np.float64)
    env = 10.0 ** (-3.0 * n / (T60 * RATE))
    h = np.zeros((lead + Lr, 2))
    h[lead:, 0] = g.standard_normal(Lr) * env * 0.2
    h[lead:, 1] = g.standard_normal(Lr) * env * 0.2 * right_gain
    h[lead, 0] += 1.0
    if delay < Lr:
        h[lead + delay, 1] += right_gain
    return h.astype(np.float32)


def envelope_rir(Lr, T60, seed):
    """Noise under a 60 dB exponential envelope alone (the t30 margin cases)"""
    g = np.random.default_rng(seed)
    env = 10.0 ** (-3.0 * np.arange(Lr, dtype=np.float64) / (T60 * RATE))
    return (g.standard_normal((Lr, 2)) * env[:, None]).astype(np.float32)


# name -> RIR [Lr, 2] fp32: the shapes at which the kernels can still go wrong
# (the float64 reference convolves a whole row through one transform, so a row's decay stays inside ~190 dB)
def cases():
    c = {}
    c["Lr1"] = np.array([[0.5, -0.25]], dtype=np.float32)
    c["Lr700"] = noise_rir(700, 0.05, 1)
    c["Lr700.silent"] = np.zeros((700, 2), dtype=np.float32)
    c["Lr700.silent_ear"] = noise_rir(700, 0.05, 8)
    c["Lr700.silent_ear"][:, 1] = 0.0
    c["two_segments_lead300"] = noise_rir(HOP + LEAD + 17 - 300, 0.3, 2, lead=300)     # Lr = 12256 + 2064 + 17: n0 > 0, two segments, a partial last bin
    c["Lr30001"] = noise_rir(30001, 0.6, 3)
    for s in range(1, 12):
        c["Lr30001.s%02d" % s] = noise_rir(30001 - 7 * s, 0.6 + 0.1 * s, 20 + s, lead=7 * s, delay=s)
    c["Lr256000"] = noise_rir(256000 - 40, 12.0, 4, lead=40)      # (80 dB over the row: the float64 convolution of the reference still resolves the tail)
    return c


def batches():
    """name -> (RIRs [..., Lr, 2] fp32, the names of its RIRs in cases()): what the GPU test analyses in one call"""
    c = cases()
    names = {"Lr1": ["Lr1"], "Lr700": ["Lr700", "Lr700.silent", "Lr700.silent_ear"], "two_segments_lead300": ["two_segments_lead300"],
             "Lr30001": ["Lr30001"] + ["Lr30001.s%02d" % s for s in range(1, 12)], "Lr256000": ["Lr256000"]}
    out = {k: (np.stack([c[n] for n in v]), v) for k, v in names.items()}
    out["Lr30001"] = (out["Lr30001"][0].reshape(2, 2, 3, 30001, 2), out["Lr30001"][1])
    return out


def decay_cases():
    """rows of float64 bins of the test's own making: name -> [nb]"""
    g = np.random.default_rng(11)
    out = {}
    for nb, T in ((1, 0.3), (44, 0.05), (300, 0.1), (1000, 0.4), (1876, 0.8), (16000, 8.0)):
        i = np.arange(nb)
        out["exp.nb%d" % nb] = 10.0 ** (-6.0 * i / (T * 1000.0)) * (0.5 + g.random(nb))
    out["zeros.nb100"] = np.zeros(100)
    tail = out["exp.nb300"].copy()
    tail[200:] = 0.0
    out["zero_tail.nb300"] = tail
    return out
