"""The Scorer's broadband ITD (m2h/audio/score.py, "ITD"), restated in numpy float64 straight from the samples, with the bound its GPU
numbers are held to and a float32 restatement that shows the bound admits a correct fp32 implementation (and rejects defective ones).
Shared by tests/test_score_itd_cpu.py and tests/test_gpu_score_itd.py; no GPU, no m2h import.  Frames, spectra and TAU_FP32 are
tests/spectral_ref.py's, the binaural signals and the windows tests/spatial_ref.py's.

Definition.  Three binaural signals per recording, raw: G = refs[target], E = est, B = mix; under alignment (region [D, L - D)) BOTH
ears of the estimate are read at ONE lag.  The spectrogram of a one-second tile is spectral_ref's (T = 32 frames).  Per tile, signal and
bin k = 0 .. 255 the cross-spectrum of the ears summed over the frames, CRE_k = sum_f Re(X_L conj X_R), CIM_k = sum_f Im(X_L conj X_R):
tile sums [J, 3, 256, 2]; a window's sums are its tiles' added in tile order.  With Phi_k = CRE_k + j CIM_k of a window,
Phat_k = Phi_k / |Phi_k| (0 where |Phi_k| = 0) and the band k = 6 .. 255,

  G[i] = (1 / 250) sum_k Re(Phat_k exp(-j 2 pi k i / (1023 . 8)))        i = -128 .. 128, the lag tau_i = i / 8 samples

The ITD is the tau_i of largest G (not |G|); among equal maxima the smallest |i|, then the negative one; in microseconds, tau . 62.5.
`peak` is that maximum.  A signal without a bin of the band at |Phi_k| > 0 has itd and peak NaN.  ORDER names the nine numbers.

Bound.  An fp32 transform of the windowed frame x_t w returns every bin within u[t] = sqrt(2) TAU_FP32 |x_t w|_2 (spectral_ref).  A cross
term, real or imaginary part of X_L conj X_R, then moves by at most b = |X_L| u_R + |X_R| u_L + u_L u_R (spatial_ref); summed over a
bin's frames and a window's tiles this is b_k, for each of CRE_k and CIM_k, so |d Phi_k| <= sqrt(2) b_k.  A unit phasor moves by at most
2 |d Phi| / |Phi| (and never by more than 2), so every value of G moves by at most

  E = (1 / 250) sum_k min(2, 2 sqrt(2) b_k / |Phi_k|)

the same for every lag.  A pick is certain where the margin -- the largest G minus the next grid value -- exceeds 2 E.
"""
import numpy as np

import spatial_ref as PR
import spectral_ref as SR
from elem_bound import TAU_FP32

TILE, T = SR.TILE, SR.T
NBINS = 256
BINS = (6, 256)
MAX_LAG, UPSAMPLE = 16, 8
H = MAX_LAG * UPSAMPLE
NL = 2 * H + 1
US_PER_STEP = 1e6 / (16000 * UPSAMPLE)
ORDER = ("itd", "itd_est", "itd_mix", "itd_err", "itd_err_base", "itd_erri", "peak", "peak_est", "peak_mix")

signals = PR.signals
window_sums = PR.window_sums


def cross_sums(XL, XR, wrong_conj=False):
    """complex [T, F] spectra of the two ears -> [256, 2] float64: (CRE, CIM) per bin, summed over the frames.  Defect: wrong_conj:
    conj X_L . X_R instead of X_L . conj X_R."""
    z = (np.conj(XL) * XR if wrong_conj else XL * np.conj(XR))[:, :NBINS].sum(axis=0)
    return np.stack([z.real, z.imag], axis=-1)


def cross_bound(fl, fr, XL, XR):
    """b_k [256] of one tile: the bound of each of CRE_k and CIM_k, from the float64 frames and spectra of the two ears"""
    u = lambda f: (np.sqrt(2.0) * TAU_FP32 * np.sqrt((f ** 2).sum(axis=1)))[:, None]   # noqa: E731   [T, 1]
    ul, ur = u(fl), u(fr)
    return (np.abs(XL) * ur + np.abs(XR) * ul + ul * ur)[:, :NBINS].sum(axis=0)


def tile_sums(sig, j):
    """(sums [3, 256, 2], bound [3, 256]) of tile j of the three binaural signals, float64"""
    sums, bound = [], []
    for xl, xr in sig:
        fl, fr = SR.frames_of(SR.second(xl, j)), SR.frames_of(SR.second(xr, j))
        XL, XR = SR.spectrum(fl), SR.spectrum(fr)
        sums.append(cross_sums(XL, XR))
        bound.append(cross_bound(fl, fr, XL, XR))
    return np.stack(sums), np.stack(bound)


def tile_sums32(sig, j, swap_ears=False, **defect):
    """the float32 restatement of tile j: an fp32 matrix product (spectral_ref.spectrum32), the epilogue in float64 from the fp32 values.
    Defects: swap_ears: every signal's ears exchanged; wrong_conj: cross_sums'."""
    out = []
    for pair in sig:
        l, r = [PR._c32(SR.spectrum32(SR.frames_of(SR.second(x, j), np.float32))) for x in pair]
        if swap_ears:
            l, r = r, l
        out.append(cross_sums(l, r, **defect))
    return np.stack(out)


def recording_sums(refs, est, mix, target=0, lag=0, D=0, lag_right=None, fp32=False):
    """one recording -> (sums [J, 3, 256, 2], bound [J, 3, 256]) float64; lag: the one lag of both ears (with D); lag_right: the defect,
    the estimate's right ear at a lag of its own; fp32: the sums of the float32 restatement instead"""
    J = -(-(refs.shape[-1] - 2 * D) // TILE)
    sig = signals(refs, est, mix, target, lag, D, lag_right)
    out = [tile_sums(sig, j) for j in range(J)]
    sums = np.stack([tile_sums32(sig, j) for j in range(J)]) if fp32 else np.stack([o[0] for o in out])
    return sums, np.stack([o[1] for o in out])


def whole_then_track(tiles, window=1, hop=1):
    """[J, ...] -> [1 + M, ...]: all tiles added in tile order, then the plan's windows"""
    return np.concatenate([window_sums(tiles, tiles.shape[0], 1), window_sums(tiles, window, hop)])


def gcc(sums, bins=BINS, phat=True, upsample=UPSAMPLE, flip=False):
    """[..., 256, 2] -> G [..., 257] float64.  Defects: bins: another band; phat=False: the weight left out (the cross-spectrum divided
    by its largest magnitude instead); upsample: the twiddle of another grid on the same 257 columns; flip: the lag's sign."""
    sums = np.asarray(sums, np.float64)
    k = np.arange(bins[0], bins[1])
    z = sums[..., bins[0]:bins[1], 0] + 1j * sums[..., bins[0]:bins[1], 1]
    mag = np.sqrt(z.real ** 2 + z.imag ** 2)
    with np.errstate(all="ignore"):
        p = np.where(mag > 0, z / np.where(mag > 0, mag, 1.0), 0.0) if phat else z / np.maximum(mag.max(axis=-1, keepdims=True), 1e-300)
    i = np.arange(-H, H + 1) * (-1 if flip else 1)
    ang = 2.0 * np.pi * ((k[:, None] * i[None, :]) % (1023 * upsample)) / (1023 * upsample)      # [k, i], reduced in integers
    return (p.real @ np.cos(ang) + p.imag @ np.sin(ang)) / float(BINS[1] - BINS[0])


def gcc_bound(sums, bound):
    """E [...]: what the bound b_k [..., 256] of the sums [..., 256, 2] lets every value of G move by"""
    mag = np.hypot(sums[..., BINS[0]:BINS[1], 0], sums[..., BINS[0]:BINS[1], 1])
    with np.errstate(all="ignore"):
        move = np.where(mag > 0, 2.0 * np.sqrt(2.0) * bound[..., BINS[0]:BINS[1]] / mag, np.where(bound[..., BINS[0]:BINS[1]] > 0, 2.0, 0.0))
    return np.minimum(2.0, move).sum(axis=-1) / float(BINS[1] - BINS[0])


def has_band(sums):
    """[..., 256, 2] -> [...] bool: some bin of the band has |Phi_k| > 0"""
    return (np.hypot(sums[..., BINS[0]:BINS[1], 0], sums[..., BINS[0]:BINS[1], 1]) > 0).any(axis=-1)


def pick(g):
    """G [..., 257] -> (i [...] int: the grid index -128 .. 128 of the largest G, ties to the smallest |i| and then the negative one;
    peak [...]; margin [...]: the largest G minus the next grid value)"""
    g = np.asarray(g, np.float64)
    order = np.array([0] + [s * m for m in range(1, H + 1) for s in (-1, 1)])           # 0, -1, +1, -2, +2, ...
    first = np.argmax(g[..., order + H], axis=-1)
    srt = np.sort(g, axis=-1)
    return order[first], srt[..., -1], srt[..., -1] - srt[..., -2]


def nine(g, has=None):
    """G [..., 3, 257] (target, estimate, mixture), has [..., 3] -> the nine numbers [..., 9] in ORDER, as the definition writes them"""
    i, peak, _ = pick(g)
    itd = i * US_PER_STEP
    if has is not None:
        itd, peak = np.where(has, itd, np.nan), np.where(has, peak, np.nan)
    err, base = np.abs(itd[..., 1] - itd[..., 0]), np.abs(itd[..., 2] - itd[..., 0])
    return np.stack([itd[..., 0], itd[..., 1], itd[..., 2], err, base, base - err, peak[..., 0], peak[..., 1], peak[..., 2]], axis=-1)


def recording(refs, est, mix, target=0, lag=0, D=0, window=1, hop=1, lag_right=None):
    """one recording, everything the GPU test compares against: {"sums" [J, 3, 256, 2], "bound" [J, 3, 256], "wsums" [1 + M, 3, 256, 2],
    "gcc" [1 + M, 3, 257], "E" [1 + M, 3], "i" [1 + M, 3] grid indices, "margin" [1 + M, 3], "nine" [1 + M, 9]}, the whole recording first"""
    sums, bound = recording_sums(refs, est, mix, target, lag, D, lag_right)
    ws, wb = whole_then_track(sums, window, hop), whole_then_track(bound, window, hop)
    g = gcc(ws)
    i, _, margin = pick(g)
    return {"sums": sums, "bound": bound, "wsums": ws, "gcc": g, "E": gcc_bound(ws, wb), "i": i, "margin": margin, "nine": nine(g, has_band(ws))}


def late(x, d):
    """x delayed by d >= 0 samples (zeros in front), the same length"""
    return np.concatenate([np.zeros(d), x[:len(x) - d]])


def fractional(x, d):
    """x delayed by d samples, d a multiple of 1 / 8, as a phase shift of the whole row's spectrum (circular)"""
    n = len(x)
    return np.fft.irfft(np.fft.rfft(x) * np.exp(-2j * np.pi * np.fft.rfftfreq(n) * d), n)


def ear_pair(x, d, gain=1.0):
    """[2, n]: the right ear is gain x the left one d samples later (d < 0: the left ear is the late one); integer d or a multiple of 1 / 8"""
    if d != int(d):
        return np.stack([x, gain * fractional(x, d)])
    d = int(d)
    return np.stack([x, gain * late(x, d)]) if d >= 0 else np.stack([late(x, -d), gain * x])


# the planted delays in samples, per recording: (the S = 3 references', the target first; the estimate's).  All on the 1 / 8-sample grid;
# +-16 sits on the edge of the lags and 17 beyond it, where the edge value is what the definition says.
PLANTED = (((16, -7, 3), 2.5), ((-16, 9, -2), 17))
GAINS = (1.0, 0.55, 0.4)


def left_lag(r, shift=0):
    """the lag of the estimate's left ear against the target's in planted(r, ..., shift): a negative delay makes the LEFT ear the late one"""
    return shift - max(0, -int(PLANTED[r][0][0])) + max(0, -int(PLANTED[r][1]))


def planted(r, L, S=3, shift=0):
    """recording r of the GPU test's batch -> refs [S, 2, L], est [2, L], mix [2, L] float32: white sources, reference s with the
    interaural delay PLANTED[r][0][s], the estimate a filtered copy of the target's source with its own delay and a little noise, moved
    `shift` samples later as a whole (alignment); the mixture is the sum of the references"""
    assert 2 <= S <= 3
    rng = np.random.default_rng(100 + r)
    n = L + 64
    src = 0.1 * rng.standard_normal((3, n))
    refs = np.stack([GAINS[s] * ear_pair(src[s], PLANTED[r][0][s], 0.8) for s in range(S)])
    refs = refs + 0.002 * rng.standard_normal(refs.shape)
    sm = np.convolve(src[0], [0.7, 0.2, 0.1])[:n]
    est = ear_pair(sm, PLANTED[r][1], 0.9) + 0.002 * rng.standard_normal((2, n))
    if shift:
        est = np.stack([late(e, shift) for e in est])
    if L % TILE == 1:                                                                   # a tail tile of one sample: positive in both ears of every signal, so
        refs[..., -1], est[..., -1] = np.abs(refs[..., -1]), np.abs(est[..., -1])       # that its G has one peak (at 0) and not a symmetric pair of them
    mix = refs.sum(axis=0)
    return refs[..., 64:].astype(np.float32), est[:, 64:].astype(np.float32), mix[:, 64:].astype(np.float32)


def tone_pair(k0, k1, d0, d1, L=TILE):
    """[2, L] float64: two tones at the centres of the bins k0 and k1 with the interaural delays d0 and d1 samples -- a band that starts
    or ends one bin off sees one tone more or one tone less"""
    t = np.arange(L + 64)
    x = [np.cos(2.0 * np.pi * k * t / 1023.0 + 0.3 * k) for k in (k0, k1)]
    return (ear_pair(x[0], d0) + ear_pair(x[1], d1))[:, 64:]


def worst(got, want, bound):
    return SR.worst(got, want, bound)


# the cases of the GPU test: (L, D, the shift of the estimate as a whole under alignment); R = 2 recordings, S = 2 or 3 each
R = 2
CASES = ((16000, 0, 0), (16001, 0, 0), (40001, 0, 0), (40001, 300, 37))
_made = {}


def case(L, D, shift, S):
    """-> (inputs: R tuples (refs, est, mix) float32, want: R dicts of recording(...) with window = hop = 1); made once, shared, read-only"""
    key = (L, D, shift, S)
    if key not in _made:
        inputs = [planted(r, L, S, shift) for r in range(R)]
        want = [recording(*inputs[r], target=0, lag=left_lag(r, shift) if D else 0, D=D) for r in range(R)]
        for a in [x for t in inputs for x in t] + [v for w in want for v in w.values()]:
            a.setflags(write=False)
        _made[key] = (inputs, want)
    return _made[key]
