"""The Scorer's alignment (m2h/audio/score.py, "Alignment"), restated in float64 and beyond: the tile correlations by direct sums, the lag
with its tie rule, the aligned scores as score_ref.score_direct_f64 on the three slices of the definition, and the error scale of a
tile's correlation.  Shared by tests/test_align_cpu.py and tests/test_gpu_align.py; no GPU, no m2h import.

Bound.  A tile's correlation is one product of the 32768-point fp32 transform; the project's bound for that product is PRODUCT_BOUND
(tests/render_ref.py), relative to the product's scale.  For a correlation the scale is its Cauchy-Schwarz bound |s_seg|_2 |x_seg|_2:
E(tile) = PRODUCT_BOUND |s_seg|_2 |x_seg|_2, and E(window) the sum over the window's tiles.
"""
import numpy as np

import score_ref as REF
from render_ref import PRODUCT_BOUND

DIRECT_MAX_D = 512         # corr_direct: np.longdouble sums up to here, float64 scipy.fft above
S = 3
R = 2

# L, tile, D, lags [recording][channel], seed, C.  The first five are the issue's table (recording 0, channel 0 carries its lag; the
# other recording and the other ear carry other lags); then tile + 2 D = 32768 exactly with Lr = tile + 1, and Lr = 2.  The planted lag
# is the reference's whole-recording lag unless the case says "recovered": False.
CASES = [
    dict(L=40001, tile=16000, D=300, lags=[[137, -41], [-300, 300]], seed=1, C=2),
    dict(L=40001, tile=16000, D=300, lags=[[-300], [299]], seed=2, C=1),
    dict(L=64384, tile=16000, D=8192, lags=[[-8000], [8192]], seed=3, C=1),
    dict(L=40, tile=7, D=3, lags=[[2, -3], [3, 0]], seed=4, C=2),
    dict(L=16065, tile=16000, D=32, lags=[[0], [-1]], seed=5, C=1),
    dict(L=32769, tile=16384, D=8192, lags=[[-8192], [4097]], seed=6, C=1),
    dict(L=8, tile=7, D=3, lags=[[1], [0]], seed=7, C=1, recovered=False),      # two samples do not determine a lag: the reference's lag counts
]


def case_id(case):
    return "L%d-tile%d-D%d-C%d" % (case["L"], case["tile"], case["D"], case["C"])


def shifted(est, lag):
    """est [..., L] moved by `lag` samples, zeros shifted in: out[t] = est[t - lag] (the correlation sum_t s[t] out[t + d] peaks at d = lag)"""
    out = np.zeros_like(est)
    L = est.shape[-1]
    if lag >= 0:
        out[..., lag:] = est[..., :L - lag]
    else:
        out[..., :L + lag] = est[..., -lag:]
    return out


_inputs = {}


def case_inputs(case):
    """-> refs [R, S, C, L], est [R, C, L] (every ear shifted by its lag), mix [R, 2, L], clean [R, C, L] (the estimate before the shift);
    fp32, made once, shared and read-only"""
    key = case_id(case) + "-%d" % case["seed"]
    if key not in _inputs:
        rows = []
        for r in range(R):
            refs, est, mix = REF.inputs(S, case["L"], case["seed"] + 50 * r, case["C"])
            moved = np.stack([shifted(est[c], case["lags"][r][c]) for c in range(case["C"])])
            rows.append((refs, moved, mix, est))
        _inputs[key] = tuple(np.stack(a) for a in zip(*rows))
        for a in _inputs[key]:
            a.setflags(write=False)
    return _inputs[key]


def tiles_of(L, D, tile):
    """[(t0, t1)] of the region [D, L - D) in coordinates of the input"""
    Lr = L - 2 * D
    return [(D + j * tile, D + min((j + 1) * tile, Lr)) for j in range(-(-Lr // tile))]


def corr_direct(s, x, D, tile, fft=None):
    """ct [J, 2 D + 1] float64: ct[j, d + D] = sum_t s[t] x[t + d], t over tile j of the region; s, x [L].  Direct sums in np.longdouble for
    D <= DIRECT_MAX_D, float64 scipy.fft above (fft=True / False forces a route)."""
    L = s.shape[-1]
    use_fft = D > DIRECT_MAX_D if fft is None else fft
    out = []
    for t0, t1 in tiles_of(L, D, tile):
        n = t1 - t0
        if use_fft:
            import scipy.fft
            nfft = scipy.fft.next_fast_len(n + 2 * D, real=True)
            Sf = scipy.fft.rfft(np.asarray(s[t0:t1], np.float64), nfft)
            Xf = scipy.fft.rfft(np.asarray(x[t0 - D:t1 + D], np.float64), nfft)
            out.append(scipy.fft.irfft(np.conj(Sf) * Xf, nfft)[:2 * D + 1])
        else:
            ss, xx = np.asarray(s[t0:t1], np.longdouble), np.asarray(x, np.longdouble)
            out.append(np.array([np.dot(ss, xx[t0 + d:t1 + d]) for d in range(-D, D + 1)], np.longdouble).astype(np.float64))
    return np.stack(out)


def tile_bound(s, x, D, tile):
    """E [J]: PRODUCT_BOUND |s_seg|_2 |x_seg|_2 per tile (x_seg: the n + 2 D samples the tile's lags read)"""
    return np.array([PRODUCT_BOUND * np.linalg.norm(np.asarray(s[t0:t1], np.float64)) * np.linalg.norm(np.asarray(x[t0 - D:t1 + D], np.float64))
                     for t0, t1 in tiles_of(s.shape[-1], D, tile)])


def windows_of(J, window=1, hop=1):
    """[(j0, j1)] tiles per window, as score_ref.plan_windows counts them"""
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    return [(min(m * hop, J), min(m * hop + window, J)) for m in range(M)]


def window_sums(per_tile, window=1, hop=1):
    """per_tile [J, ...] -> [1 + M, ...]: the whole recording, then every window: its tiles added in tile order"""
    J = per_tile.shape[0]
    zero = np.zeros_like(per_tile[0])
    return np.stack([sum(per_tile[j0:j1], zero) for j0, j1 in [(0, J)] + windows_of(J, window, hop)])


def lag_of(c):
    """c [..., 2 D + 1] -> the lag of largest |c|: among equal maxima the smallest |d|, then the negative one"""
    K = c.shape[-1]
    D = K // 2
    order = sorted(range(-D, D + 1), key=lambda d: (abs(d), d))                         # 0, -1, +1, -2, +2, ...
    a = np.abs(np.asarray(c))[..., [d + D for d in order]]
    return np.asarray(order)[np.argmax(a, axis=-1)]                                     # np.argmax: the first maximum


def margin_of(c):
    """largest |c| minus second largest |c| along the last axis"""
    a = np.sort(np.abs(np.asarray(c)), axis=-1)
    return a[..., -1] - a[..., -2]


def score_aligned_f64(refs, est, mix, D, lags, target=0, tile=16000, window=1, hop=1):
    """One recording: refs [S, C, L], est [C, L], mix [2, L], lags [C] -> (whole [C, 11], track [C, M, 11]): score_direct_f64 on
    refs[..., D : L - D], mix[..., D : L - D] and est[c, D + lag_c : L - D + lag_c]"""
    L = refs.shape[-1]
    moved = np.stack([est[c, D + int(lags[c]):L - D + int(lags[c])] for c in range(est.shape[0])])
    return REF.score_direct_f64(refs[..., D:L - D], moved, mix[..., D:L - D], target, tile, window, hop)
