"""The Scorer's STFT distance (m2h/audio/score.py, "Spectral"), restated in numpy float64 straight from the samples, with the bound its
GPU sums are held to and a float32 restatement that shows the bound admits a correct fp32 implementation (and rejects defective ones).
Shared by tests/test_score_spectral_cpu.py and tests/test_gpu_score_spectral.py; no GPU, no m2h import.

Definition.  A tile is one second, 16000 samples, zero-extended where the recording ends; it is reflect-padded by 511 inside the tile,
cut into T = 32 frames of 1023 samples every 512, multiplied by float32(periodic Hann) and transformed by a 1023-point DFT, bins
0 .. 511 (F = 512).  With G, E, B the spectra of the raw target, estimate and baseline, the seven sums over a tile's F T bins:

  0 |G|^2   1 |E|^2   2 |B|^2   3 (|E| - |G|)^2   4 |E - G|^2   5 (|B| - |G|)^2   6 |B - G|^2

Bound.  An fp32 transform of the windowed frame x_t w returns every bin within u_x[t] = sqrt(2) TAU_FP32 |x_t w|_2 (tests/elem_bound.py:
the error of a sum does not shrink when its terms cancel; sqrt(2) for the real and the imaginary part together).  A magnitude moves by
no more than its bin does, so a term (p - q)^2 moves by at most 2 |p - q| (u_p + u_q) + (u_p + u_q)^2; the bound of a sum is that,
summed over t and k, with q = 0 and u_q = 0 for the three energies and |E - G| in place of ||E| - |G|| for the complex sums.
"""
import numpy as np

from elem_bound import TAU_FP32

TILE, NFFT, HOP, PAD, F, T = 16000, 1023, 512, 511, 512, 32
ORDER = ("stft_l2", "stft_l2_complex", "sc", "stft_l2_base", "stft_l2_complex_base", "sc_base", "stft_l2i", "stft_l2_complexi")
CLICKS = (0, 3, 509, 515, 1021, 8191, 15490, 15997, 15999)


def hann32(symmetric=False):
    """the periodic Hann window of 1023 points rounded to float32 (symmetric=True: the defect)"""
    n = np.arange(NFFT)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (NFFT - 1 if symmetric else NFFT))).astype(np.float32)


def second(x, j):
    """tile j of the row x, zero-extended to 16000 samples"""
    seg = np.asarray(x[j * TILE:(j + 1) * TILE])
    return np.concatenate([seg, np.zeros(TILE - len(seg), seg.dtype)])


def frames_of(x, dtype=np.float64, window=None, pad_mode="reflect", offset=0, reflect_at=None):
    """[T, 1023] windowed frames of one second x (16000 samples).  Defects: another window or padding mode; offset: frames start that
    many samples late; reflect_at = n: a short tile of n samples reflected at its own end instead of zero-extended first."""
    w = hann32() if window is None else window
    if reflect_at is None:
        xp = np.pad(np.asarray(x, dtype), (PAD - offset, PAD + offset), mode=pad_mode)
    else:
        xp = np.pad(np.asarray(x[:reflect_at], dtype), PAD, mode=pad_mode)
        xp = np.concatenate([xp, np.zeros(TILE + 2 * PAD - len(xp), dtype)])
    return np.stack([xp[t * HOP:t * HOP + NFFT] for t in range(T)]) * w.astype(dtype)


def spectrum(fr):
    """[T, 1023] float64 frames -> [T, F] complex128"""
    return np.fft.fft(np.asarray(fr, np.float64), axis=1)[:, :F]


_dft32 = []


def spectrum32(fr):
    """[T, 1023] float32 frames -> (re, im) float32 [T, F]: a float32 matrix product against the float32-rounded DFT matrix"""
    if not _dft32:
        ang = 2.0 * np.pi * ((np.arange(NFFT)[:, None] * np.arange(F)[None, :]) % NFFT) / NFFT
        _dft32.extend([np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32)])
    fr = np.asarray(fr, np.float32)
    return fr @ _dft32[0], fr @ _dft32[1]


def seven(G, E, B):
    """the seven sums of one tile from complex128 spectra"""
    aG, aE, aB = np.abs(G), np.abs(E), np.abs(B)
    return np.array([(aG ** 2).sum(), (aE ** 2).sum(), (aB ** 2).sum(), ((aE - aG) ** 2).sum(), (np.abs(E - G) ** 2).sum(),
                     ((aB - aG) ** 2).sum(), (np.abs(B - G) ** 2).sum()])


def seven32(g, e, b):
    """the same from (re, im) float32 pairs: magnitudes and differences in float32, every square converted to float64 before it is added"""
    sq = lambda v: (np.asarray(v, np.float64) ** 2).sum()                              # noqa: E731
    mag = lambda p: np.sqrt(p[0] * p[0] + p[1] * p[1], dtype=np.float32)              # noqa: E731
    mg, me, mb = mag(g), mag(e), mag(b)
    return np.array([sq(g[0]) + sq(g[1]), sq(e[0]) + sq(e[1]), sq(b[0]) + sq(b[1]), sq(me - mg), sq(e[0] - g[0]) + sq(e[1] - g[1]),
                     sq(mb - mg), sq(b[0] - g[0]) + sq(b[1] - g[1])])


def seven_bound(fg, fe, fb, G, E, B):
    """the bound of each of the seven sums (module docstring) from the float64 frames and spectra of one tile"""
    u = lambda fr: (np.sqrt(2.0) * TAU_FP32 * np.sqrt((fr ** 2).sum(axis=1)))[:, None]   # noqa: E731   [T, 1]
    ug, ue, ub = u(fg), u(fe), u(fb)
    term = lambda d, v: (2.0 * d * v + np.broadcast_to(v * v, d.shape)).sum()           # noqa: E731   (v is per frame, d per bin)
    aG, aE, aB = np.abs(G), np.abs(E), np.abs(B)
    return np.array([term(aG, ug), term(aE, ue), term(aB, ub), term(np.abs(aE - aG), ue + ug), term(np.abs(E - G), ue + ug),
                     term(np.abs(aB - aG), ub + ug), term(np.abs(B - G), ub + ug)])


def signals(refs, est, mix, c, target=0, lag=0, D=0):
    """one recording: refs [S, C, L], est [C, L], mix [2, L] -> the raw rows (g, e, b) of channel c in float64, over the region [D, L - D)
    with the estimate read `lag` samples later"""
    L = refs.shape[-1]
    f = lambda a: np.asarray(a, np.float64)                                             # noqa: E731
    g, e = f(refs[target, c, D:L - D]), f(est[c, D + lag:L - D + lag])
    b = f(mix[c, D:L - D]) if refs.shape[1] == 2 else 0.5 * (f(mix[0, D:L - D]) + f(mix[1, D:L - D]))
    return g, e, b


def tile_sums(g, e, b, j):
    """(sums [7], bound [7]) of tile j of the rows g, e, b, float64"""
    fr = [frames_of(second(x, j)) for x in (g, e, b)]
    sp = [spectrum(f) for f in fr]
    return seven(*sp), seven_bound(*fr, *sp)


def tile_sums32(g, e, b, j, **defect):
    """the float32 restatement of tile j; keyword arguments of frames_of plant a defect"""
    return seven32(*[spectrum32(frames_of(second(x, j), np.float32, **defect)) for x in (g, e, b)])


def recording_sums(refs, est, mix, target=0, lag=None, D=0):
    """one recording -> (sums [C, J, 7], bound [C, J, 7]) float64; lag: one int per channel (with D)"""
    C = refs.shape[1]
    J = -(-(refs.shape[-1] - 2 * D) // TILE)
    out = [[tile_sums(*signals(refs, est, mix, c, target, 0 if lag is None else lag[c], D), j) for j in range(J)] for c in range(C)]
    return np.array([[o[0] for o in row] for row in out]), np.array([[o[1] for o in row] for row in out])


def metrics(sums, Q):
    """the eight numbers in ORDER from window sums [..., 7] and the tile count Q, float64, as the definition writes them"""
    sums = np.asarray(sums, np.float64)
    with np.errstate(all="ignore"):
        den = 2.0 * F * T * np.asarray(Q, np.float64)
        l2, l2c, sc = sums[..., 3] / den, sums[..., 4] / den, np.sqrt(sums[..., 3] / sums[..., 0])
        l2b, l2cb, scb = sums[..., 5] / den, sums[..., 6] / den, np.sqrt(sums[..., 5] / sums[..., 0])
    return np.stack([l2, l2c, sc, l2b, l2cb, scb, l2b - l2, l2cb - l2c], axis=-1)


def metrics_bound(sums, bound, Q):
    """the bound of stft_l2, stft_l2_complex, stft_l2_base, stft_l2_complex_base (columns 0, 1, 3, 4 of ORDER) that follows from the sums'"""
    den = 2.0 * F * T * np.asarray(Q, np.float64)
    return np.stack([bound[..., 3] / den, bound[..., 4] / den, bound[..., 5] / den, bound[..., 6] / den], axis=-1)


def window_sums(tiles, window=1, hop=1):
    """[..., J, 7] -> ([..., M, 7] a window's tiles added in tile order, Q [M]) by the issue's plan (restated, not imported)"""
    J = tiles.shape[-2]
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    spans = [(min(m * hop, J), min(m * hop + window, J)) for m in range(M)]
    out = []
    for j0, j1 in spans:
        s = np.zeros(tiles.shape[:-2] + (7,))
        for j in range(j0, j1):
            s = s + tiles[..., j, :]
        out.append(s)
    return np.stack(out, axis=-2), np.array([j1 - j0 for j0, j1 in spans], np.float64)


def clicks(seed=0, L=TILE):
    """-> refs [1, 1, L], est [1, L], mix [2, L] float32: a target of isolated samples (frame placement, padding and the window's ends
    are invisible on noise-like inputs and visible here), an estimate 0.8 x that plus 0.002 noise and one extra click, a mixture of the
    target plus 0.05 noise"""
    r = np.random.default_rng(seed)
    g = np.zeros(TILE)
    g[list(CLICKS)] = r.uniform(0.3, 0.9, len(CLICKS)) * np.where(r.uniform(size=len(CLICKS)) < 0.5, -1.0, 1.0)
    e = 0.8 * g + 0.002 * r.standard_normal(TILE)
    e[700] += 0.4
    mix = np.stack([g + 0.05 * r.standard_normal(TILE), g + 0.05 * r.standard_normal(TILE)])
    return g[None, None, :L].astype(np.float32), e[None, :L].astype(np.float32), mix[:, :L].astype(np.float32)


def fold_on_the_table(x, table):
    """one second x -> (re, im) float32 [T, F] the way m2h_score_spectral and m2h_score_spatial compute them: raw frames, x[n] +- x[1023 - n]
    in float32, a float32 product against the rows n = 0 .. 511 of table = m2h.audio.score.spectral_table()"""
    t = table                                                                           # [bt, ks, q, l]
    assert t.dtype == np.float32 and t.shape == (32, 128, 2, 64)
    t = t.reshape(32, 128, 2, 4, 16).transpose(2, 1, 3, 0, 4).reshape(2, 512, 512)       # [q, n = 4 ks + (l >> 4), k = 16 bt + (l & 15)]
    xp = np.pad(np.asarray(x, np.float32), PAD, mode="reflect")
    fr = np.stack([xp[f * HOP:f * HOP + NFFT + 1] for f in range(T)])                   # (sample 1023 is the partner of n = 0, whose table row is 0)
    lo, hi = fr[:, :512], fr[:, :511:-1]                                                # x[n] and x[1023 - n], n = 0 .. 511
    return (lo + hi) @ t[0], (lo - hi) @ t[1]


def worst(got, want, bound):
    """the largest |got - want| / bound; a difference where the bound is 0 counts as inf"""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(all="ignore"):
        q = np.where(d == 0, 0.0, d / bound)
    return float(np.max(q))
