"""The Scorer's interaural cues (m2h/audio/score.py, "Spatial"), restated in numpy float64 straight from the samples, with the bound its
GPU sums are held to and a float32 restatement that shows the bound admits a correct fp32 implementation (and rejects defective ones).
Shared by tests/test_score_spatial_cpu.py and tests/test_gpu_score_spatial.py; no GPU, no m2h import.  Frames, spectra, the signals of
an ear and TAU_FP32 are tests/spectral_ref.py's.

Definition.  The spectrogram of a one-second tile is spectral_ref's (T = 32 frames, F = 512 bins).  NB = 32 bands of 16 bins, band j =
bins 16 j .. 16 j + 15.  Three binaural signals per recording, raw: G = refs[target], E = est, B = mix.  With X_L, X_R the two ears'
spectra of a signal, a tile's four sums over a band's 16 bins x 32 frames:

  0 PL = sum |X_L|^2   1 PR = sum |X_R|^2   2 CRE = sum Re(X_L conj X_R)   3 CIM = sum Im(X_L conj X_R)

tile sums [J, 3, 32, 4]; a window's sums are its tiles' added in tile order.  Under alignment (region [D, L - D)) BOTH ears of the
estimate are read at ONE lag.  Cues per signal and band: ILD = 10 log10(PL / PR), IPD = atan2(CIM, CRE), IC = |CRE + i CIM| /
sqrt(PL PR).  Errors: means over bands weighted by w_j = PL_G + PR_G, over the bands in which w_j > 0 and PL, PR of G and of the signal
compared are > 0 (NaN if there is none); IPD differences wrapped to (-pi, pi] and taken over the bands 0 .. 5 only.  ORDER names the nine.

Bound.  An fp32 transform of the windowed frame x_t w returns every bin within u_x[t] = sqrt(2) TAU_FP32 |x_t w|_2 (spectral_ref).  An
energy term |X|^2 then moves by at most 2 |X| u + u^2; a cross term, real or imaginary part of X_L conj X_R, by at most
|X_L| u_R + |X_R| u_L + u_L u_R (|(a + da) conj (b + db) - a conj b| <= |a| |db| + |b| |da| + |da| |db|).  The bound of a band sum is
that summed over its bins and frames.  The products and sums of the epilogue are float64 and add nothing at this scale.
"""
import numpy as np

import spectral_ref as SR
from elem_bound import TAU_FP32

TILE, F, T = SR.TILE, SR.F, SR.T
NB, BW, IPD_BANDS = 32, 16, 6
ORDER = ("ild_err", "ipd_err", "ic_err", "ild_err_base", "ipd_err_base", "ic_err_base", "ild_erri", "ipd_erri", "ic_erri")


def band_sums(XL, XR, edge=0, abs_cross=False, wrong_conj=False):
    """complex [T, F] spectra of the two ears -> [32, 4] float64.  Defects: edge = 1: every band starts one bin late (the last one is a
    bin short); abs_cross: the cross term summed as |L| |R|; wrong_conj: conj X_L . X_R instead of X_L . conj X_R."""
    cross = np.abs(XL) * np.abs(XR) + 0j if abs_cross else (np.conj(XL) * XR if wrong_conj else XL * np.conj(XR))
    terms = np.stack([np.abs(XL) ** 2, np.abs(XR) ** 2, cross.real, cross.imag], axis=-1)          # [T, F, 4]
    if edge:
        terms = np.concatenate([terms[:, edge:], np.zeros((T, edge, 4))], axis=1)
    return terms.reshape(T, NB, BW, 4).sum(axis=(0, 2))


def band_bound(fl, fr, XL, XR):
    """the bound of each of the [32, 4] sums (module docstring) from the float64 frames and spectra of the two ears of one tile"""
    u = lambda f: (np.sqrt(2.0) * TAU_FP32 * np.sqrt((f ** 2).sum(axis=1)))[:, None]   # noqa: E731   [T, 1]
    ul, ur = u(fl), u(fr)
    aL, aR = np.abs(XL), np.abs(XR)
    cross = aL * ur + aR * ul + ul * ur
    terms = np.stack([2.0 * aL * ul + ul * ul, 2.0 * aR * ur + ur * ur, cross, cross], axis=-1)
    return terms.reshape(T, NB, BW, 4).sum(axis=(0, 2))


def signals(refs, est, mix, target=0, lag=0, D=0, lag_right=None):
    """one recording: refs [S, 2, L], est [2, L], mix [2, L] -> ((gL, gR), (eL, eR), (bL, bR)) raw float64 rows over the region [D, L - D),
    both ears of the estimate read `lag` samples later (lag_right: the defect, the right ear at a lag of its own)"""
    ears = [SR.signals(refs, est, mix, c, target, lag if c == 0 or lag_right is None else lag_right, D) for c in range(2)]
    return tuple((ears[0][x], ears[1][x]) for x in range(3))


def tile_sums(sig, j):
    """(sums [3, 32, 4], bound [3, 32, 4]) of tile j of the three binaural signals, float64"""
    sums, bound = [], []
    for xl, xr in sig:
        fl, fr = SR.frames_of(SR.second(xl, j)), SR.frames_of(SR.second(xr, j))
        XL, XR = SR.spectrum(fl), SR.spectrum(fr)
        sums.append(band_sums(XL, XR))
        bound.append(band_bound(fl, fr, XL, XR))
    return np.stack(sums), np.stack(bound)


def _c32(p):
    """(re, im) float32 -> complex128: the epilogue's products are float64 of the fp32 values"""
    return np.asarray(p[0], np.float64) + 1j * np.asarray(p[1], np.float64)


def sums32(spectra, swap_ears=False, cross_pair=False, **defect):
    """[3, 32, 4] from the (re, im) float32 spectra ((GL, GR), (EL, ER), (BL, BR)).  Defects: swap_ears: every signal's ears exchanged;
    cross_pair: the estimate's right ear paired with the TARGET's left; the rest are band_sums'."""
    out = []
    for x, (l, r) in enumerate(spectra):
        if cross_pair and x == 1:
            l = spectra[0][0]
        if swap_ears:
            l, r = r, l
        out.append(band_sums(_c32(l), _c32(r), **defect))
    return np.stack(out)


def tile_sums32(sig, j, **defect):
    """the float32 restatement of tile j: an fp32 matrix product (spectral_ref.spectrum32), the epilogue in float64 from the fp32 values"""
    return sums32([[SR.spectrum32(SR.frames_of(SR.second(x, j), np.float32)) for x in pair] for pair in sig], **defect)


def recording_sums(refs, est, mix, target=0, lag=0, D=0):
    """one recording -> (sums [J, 3, 32, 4], bound [J, 3, 32, 4]) float64; lag: the one lag of both ears (with D)"""
    J = -(-(refs.shape[-1] - 2 * D) // TILE)
    sig = signals(refs, est, mix, target, lag, D)
    out = [tile_sums(sig, j) for j in range(J)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def window_sums(tiles, window=1, hop=1):
    """[J, ...] -> [M, ...]: a window's tiles added in tile order, by the issue's plan (restated, not imported)"""
    J = tiles.shape[0]
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    out = []
    for j0, j1 in [(min(m * hop, J), min(m * hop + window, J)) for m in range(M)]:
        s = np.zeros(tiles.shape[1:])
        for j in range(j0, j1):
            s = s + tiles[j]
        out.append(s)
    return np.stack(out)


def cues(sums):
    """[..., 3, 32, 4] -> [..., 3, 32, 3]: ILD (dB), IPD (rad), IC"""
    sums = np.asarray(sums, np.float64)
    pl, pr, z = sums[..., 0], sums[..., 1], sums[..., 2] + 1j * sums[..., 3]
    with np.errstate(all="ignore"):
        return np.stack([10.0 * np.log10(pl / pr), np.angle(z), np.abs(z) / np.sqrt(pl * pr)], axis=-1)


def wrap(d):
    """to (-pi, pi]"""
    return d - 2.0 * np.pi * np.ceil((d - np.pi) / (2.0 * np.pi))


def weights(sums):
    """w [..., 32] = PL_G + PR_G"""
    sums = np.asarray(sums, np.float64)
    return sums[..., 0, :, 0] + sums[..., 0, :, 1]


def valid(sums, x):
    """[..., 32] bool: the bands that enter the errors of signal x"""
    sums = np.asarray(sums, np.float64)
    ok = lambda s: (sums[..., s, :, 0] > 0) & (sums[..., s, :, 1] > 0)                  # noqa: E731
    return (weights(sums) > 0) & ok(0) & ok(x)


def metrics(sums):
    """[..., 3, 32, 4] -> the nine numbers [..., 9] in ORDER, float64, as the definition writes them"""
    sums = np.asarray(sums, np.float64)
    c, w = cues(sums), weights(sums)
    err = []
    with np.errstate(all="ignore"):
        for x in (1, 2):
            ok = valid(sums, x)
            for k, bands in ((0, NB), (1, IPD_BANDS), (2, NB)):
                d = c[..., x, :, k] - c[..., 0, :, k]
                d = np.abs(wrap(d) if k == 1 else d)
                m = ok[..., :bands]
                err.append(np.where(m, w[..., :bands] * d[..., :bands], 0.0).sum(axis=-1) / np.where(m, w[..., :bands], 0.0).sum(axis=-1))
    return np.stack(err + [err[3 + k] - err[k] for k in range(3)], axis=-1)


def ild_bound(sums, bound):
    """what the bound of the sums lets ILD [..., 3, 32] move by, dB: |d log10(PL / PR)| <= (bPL / (PL - bPL) + bPR / (PR - bPR)) / ln 10
    (the mean value theorem on log over [P - b, P + b]); inf where a bound reaches its sum"""
    pl, pr, bl, br = sums[..., 0], sums[..., 1], bound[..., 0], bound[..., 1]
    with np.errstate(all="ignore"):
        d = 10.0 / np.log(10.0) * (bl / (pl - bl) + br / (pr - br))
    return np.where((bl < pl) & (br < pr), d, np.inf)


def cues_bound(sums, bound):
    """what the bound of the sums lets the cues [..., 3, 32, 3] move by, rigorously; inf where a bound reaches its sum.
    ILD: ild_bound.  IPD: a vector z moved by at most d = |(bCRE, bCIM)| < |z| turns by at most asin(d / |z|).
    IC = |z| / sqrt(PL PR) <= (|z| + d) / sqrt((PL - bPL)(PR - bPR)), and the move downwards is smaller."""
    pl, pr, bl, br = sums[..., 0], sums[..., 1], bound[..., 0], bound[..., 1]
    n, d = np.hypot(sums[..., 2], sums[..., 3]), np.hypot(bound[..., 2], bound[..., 3])
    with np.errstate(all="ignore"):
        ipd = np.where(d < n, np.arcsin(np.minimum(d / n, 1.0)), np.inf)
        ic = np.where((bl < pl) & (br < pr), (n + d) / np.sqrt((pl - bl) * (pr - br)) - n / np.sqrt(pl * pr), np.inf)
    return np.stack([ild_bound(sums, bound), ipd, ic], axis=-1)


def metrics_bound(sums, bound):
    """what the bound of the sums lets the nine numbers [..., 9] move by.  An error is m = sum w d / sum w over its valid bands, with
    d = |cue_x - cue_G|: d moves by at most the two cues' bounds, a weighted mean of which is at most their largest; the weights w move by
    bw = bPL_G + bPR_G, which moves a weighted mean of values in [0, max d] by at most 2 max d . sum bw / (sum w - sum bw).  The
    improvements move by the two errors' bounds added.  (The valid bands are taken from `sums`.)"""
    sums, bound = np.asarray(sums, np.float64), np.asarray(bound, np.float64)
    c, cb, w = cues(sums), cues_bound(sums, bound), weights(sums)
    bw = bound[..., 0, :, 0] + bound[..., 0, :, 1]
    out = []
    with np.errstate(all="ignore"):
        for x in (1, 2):
            ok = valid(sums, x)
            for k, bands in ((0, NB), (1, IPD_BANDS), (2, NB)):
                m = ok[..., :bands]
                d = c[..., x, :bands, k] - c[..., 0, :bands, k]
                d = np.where(m, np.abs(wrap(d) if k == 1 else d), 0.0)
                move = np.where(m, cb[..., x, :bands, k] + cb[..., 0, :bands, k], 0.0).max(axis=-1)
                sw, sbw = np.where(m, w[..., :bands], 0.0).sum(axis=-1), np.where(m, bw[..., :bands], 0.0).sum(axis=-1)
                out.append(move + np.where(sbw < sw, 2.0 * d.max(axis=-1) * sbw / (sw - sbw), np.inf))
    return np.stack(out + [out[3 + k] + out[k] for k in range(3)], axis=-1)


def binaural(seed=0, L=TILE, delay=5, gain=0.5):
    """-> refs [1, 2, L], est [2, L], mix [2, L] float32 with a clear spatial image: the target's left ear is noise, its right ear `gain`
    x the left `delay` samples later plus independent noise at -20 dB; the estimate is a differently filtered copy (another gain and
    delay, a little noise), the mixture the target plus an interferer on the other side"""
    r = np.random.default_rng(seed)
    n = L + 64
    src, other = 0.1 * r.standard_normal(n), 0.1 * r.standard_normal(n)
    late = lambda x, d: np.concatenate([np.zeros(d), x[:n - d]])                        # noqa: E731
    g = np.stack([src, gain * late(src, delay) + 0.01 * r.standard_normal(n)])
    sm = np.convolve(src, [0.6, 0.3, 0.1])[:n]
    e = np.stack([0.9 * sm, 0.7 * late(sm, 2) + 0.002 * r.standard_normal(n)])
    b = g + np.stack([0.4 * late(other, 6), other])
    return g[None, :, 64:].astype(np.float32), e[:, 64:].astype(np.float32), b[:, 64:].astype(np.float32)


def click_pairs(seed=0, L=TILE):
    """spectral_ref.clicks made binaural: -> refs [1, 2, L], est [2, L], mix [2, L]; the right ears are the left ones 3 samples later at
    0.7 x (estimate: 2 samples, 0.8 x), so frame placement shows in the cross terms too"""
    refs, est, mix = SR.clicks(seed)
    late = lambda x, d, a: np.concatenate([np.zeros(d, np.float32), (a * x[:TILE - d]).astype(np.float32)])   # noqa: E731
    g = np.stack([refs[0, 0], late(refs[0, 0], 3, 0.7)])
    e = np.stack([est[0], late(est[0], 2, 0.8)])
    return g[None, :, :L], e[:, :L], mix[:, :L]


def worst(got, want, bound):
    return SR.worst(got, want, bound)
