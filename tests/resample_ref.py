"""CPU statement of m2h.audio.resample's definition in numpy float64, in the direct and in the polyphase form.  Helper module, no tests.

    g = gcd(f_in, f_out), up = f_out / g, down = f_in / g, half = 10 * max(up, down), N = 2 * half + 1
    c = 1 / max(up, down), m = arange(N) - half, h = c * sinc(c * m) * kaiser(N, 5.0), h /= h.sum(), h *= up
    y[n] = sum_j x[j] * h[n * down - j * up + half],  0 <= n < ceil(L_in * up / down),  x zero outside [0, L_in)
    polyphase: t = n * down + half, p = t mod up, j0 = t div up, y[n] = sum_{k < T} G[p][k] * x[j0 - k], G[p][k] = h[p + k * up]
"""
import math

import numpy as np

RATES = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 44100), (16000, 48000)]
TAPS = {(48000, 16000): 61, (44100, 16000): 56, (22050, 16000): 28, (8000, 16000): 21, (16000, 44100): 21, (16000, 48000): 21}


def ratio(f_in, f_out):
    g = math.gcd(f_in, f_out)
    return f_out // g, f_in // g


def taps(f_in, f_out):
    """(up, down, half, h float64)"""
    up, down = ratio(f_in, f_out)
    half = 10 * max(up, down)
    n = 2 * half + 1
    c = 1.0 / max(up, down)
    m = np.arange(n) - half
    h = c * np.sinc(c * m) * np.kaiser(n, 5.0)
    h /= h.sum()
    h *= up
    return up, down, half, h


def out_len(L, up, down):
    return -(-L * up // down)


def direct(x, h, up, down, half):
    """The defining sum over rows x [rows, L_in] in float64, term by term: every (n, j) pair whose tap index lies inside h."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    rows, L = x.shape
    Lo = out_len(L, up, down)
    y = np.zeros((rows, Lo))
    j = np.arange(L, dtype=np.int64)
    for n0 in range(0, Lo, 256):
        n = np.arange(n0, min(n0 + 256, Lo), dtype=np.int64)
        i = n[:, None] * down - j[None, :] * up + half
        H = np.where((i >= 0) & (i <= 2 * half), h[np.clip(i, 0, 2 * half)], 0.0)      # [n, j]
        y[:, n0:n0 + len(n)] = x @ H.T
    return y


def polyphase(x, h, up, down, half, n_lo=0, n_hi=None):
    """The polyphase form for outputs [n_lo, n_hi) of rows x [rows, L_in], float64."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    rows, L = x.shape
    Lo = out_len(L, up, down)
    n_hi = Lo if n_hi is None else n_hi
    T = -(-len(h) // up)
    hp = np.zeros(T * up)
    hp[:len(h)] = h
    G = hp.reshape(T, up).T                            # G[p][k] = h[p + k up]
    n = np.arange(n_lo, n_hi, dtype=np.int64)
    t = n * down + half
    p, j0 = t % up, t // up
    y = np.zeros((rows, len(n)))
    for k in range(T):
        j = j0 - k
        ok = (j >= 0) & (j < L)
        y += G[p, k] * np.where(ok, x[:, np.clip(j, 0, L - 1)], 0.0)
    return y


def scipy_resample(x, up, down):
    from scipy.signal import resample_poly
    return resample_poly(np.asarray(x, np.float64), up, down, axis=-1, window=("kaiser", 5.0), padtype="constant")


def tone_noise(rows, L, seed, rate=16000):
    """separate_ref.tone_noise's signal over plain rows: noise (sigma 0.05) plus one tone per row."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / float(rate)
    w = rng.standard_normal((rows, L)) * 0.05
    for r in range(rows):
        w[r] += 0.3 * np.sin(2 * np.pi * rng.uniform(100, 4000) * t + rng.uniform(0, 6))
    return w.astype(np.float32)


def rel_l1(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))
