"""CPU reference of m2h.separate with overlapped, cross-faded segments (overlap = k, H = 16000 / k), built from tests/separate_ref.py:
chain c (the segments s = c, c + k, ...) is the plain path applied to wave[:, :, c * H:], and the output is the cross-fade of the k
chains' waveforms with w[t] = sin^2(pi (t + 1/2) / 16000), weighted in float64.  Helper module, no tests."""
import numpy as np

import separate_ref as REF

SEG = REF.SEG
OVERLAPS = (1, 2, 4)


def window():
    """The cross-fade window as the definition states it: float64 on the host, rounded once to fp32 (returned as float64 values)."""
    t = np.arange(SEG, dtype=np.float64)
    return (np.sin(np.pi * (t + 0.5) / SEG) ** 2).astype(np.float32).astype(np.float64)


def n_segments(L, overlap):
    return -(-L // (SEG // overlap))


def chains(L, overlap):
    """The chains that exist for a recording of L samples: c with c * H < L."""
    H = SEG // overlap
    return [c for c in range(overlap) if c * H < L]


def crossfade(ys, L, overlap):
    """ys[c]: chain c's waveform [R, L - c * H] (its one-second segments concatenated and cut), for c in chains(L, overlap).
    y[n] = sum_c (w[(n - c H) mod 16000] / W[n]) * ys[c][n - c H], W[n] = the sum of those weights; float64, returned as float32."""
    H = SEG // overlap
    w = window()
    R = ys[0].shape[0]
    weights = np.zeros((len(ys), L))
    for c, yc in enumerate(ys):
        assert yc.shape == (R, L - c * H)
        weights[c, c * H:] = w[np.arange(L - c * H) % SEG]
    W = weights.sum(0)
    assert (W > 0).all()
    y = np.zeros((R, L))
    for c, yc in enumerate(ys):
        y[:, c * H:] += (weights[c, c * H:] / W[c * H:]) * yc.astype(np.float64)
    return y.astype(np.float32)


def interleave(parts, L, overlap):
    """parts[c]: chain c's per-segment array [R, S_c, ...]  ->  [R, S', ...] in segment order: out[:, c + j * k] = parts[c][:, j]."""
    S = n_segments(L, overlap)
    out = np.zeros(parts[0].shape[:1] + (S,) + parts[0].shape[2:], parts[0].dtype)
    for c, p in enumerate(parts):
        assert p.shape[1] == len(range(c, S, overlap))
        out[:, c::overlap] = p
    return out


def separate(sd, wave, target_class, use_memory, overlap):
    """As separate_ref.separate, with `overlap` segments over every sample.  Returns (y [R, L], P [R, S', 512, 32],
    phasor [R, S', 512, 32] complex), S' = ceil(L / H), P and the phasor in segment order."""
    assert overlap in OVERLAPS
    L = wave.shape[2]
    H = SEG // overlap
    ys, Ps, phs = [], [], []
    for c in chains(L, overlap):
        y, P, ph = REF.separate(sd, np.ascontiguousarray(wave[:, :, c * H:]), target_class, use_memory)
        ys.append(y)
        Ps.append(P)
        phs.append(ph)
    return crossfade(ys, L, overlap), interleave(Ps, L, overlap), interleave(phs, L, overlap)
