"""The Scorer's float64 definition, restated directly: every window scored through oracle.np_scale_bss_eval_helper (the reference's
scale_bss_eval_helper for any number of sources) on mean-removed float64 copies of the window's samples, as preprocess + scale_bss_eval
score one clip.  Shared by tests/test_score_cpu.py and tests/test_gpu_score.py; no GPU, no m2h import.

Inputs (`inputs`): amplitude-modulated tones plus noise plus an offset per source; the mixture carries a noise term of its own (`nz`),
which keeps it out of the references' span -- without it SI-SARi is rounding noise; everything rounded to fp32.
"""
import numpy as np

import m2h_oracle as O

SR = 16000.0
WELL = (0, 3, 4, 5, 6, 7, 8)      # si_sdr, sd_sdr, snr, srr, si_sdri, sd_sdri, snri: well conditioned for S = 1 too (tests/test_gpu_eval_metrics.py)
ALL = tuple(range(11))
TOL_ALGEBRA = 1e-9                # dB: float64 Gram algebra against the direct float64 formulas (measured: 3.5e-10 at worst)
TOL_GPU = 1e-6                    # dB: the GPU's scores against the direct float64 formulas
TOL_DEFECT = 1e-6                 # dB: what a defective scorer must miss by


def inputs(S, L, seed, C=1, snr43=False):
    """-> refs [S, C, L], est [C, L], mix [2, L], fp32.  snr43: an estimate at about 43 dB SI-SDR instead of about 12 dB."""
    r = np.random.default_rng(seed)
    t = np.arange(L) / SR
    refs = np.stack([np.stack([0.2 * np.sin(2 * np.pi * r.uniform(200, 3000) * t) * (1 + 0.5 * np.sin(2 * np.pi * r.uniform(0.3, 2) * t))
                               + 0.05 * r.standard_normal(L) + 0.01 * (i + 1) for _ in range(C)]) for i in range(S)])
    nz = 0.02 * r.standard_normal(L)
    w = np.linspace(0.6, 1.3, S)
    mix = np.stack([refs[:, 0].mean(axis=0) + 0.003 + nz, (w[:, None] * refs[:, C - 1]).sum(axis=0) / S - 0.002 - 0.5 * nz])
    second = refs[1] if S > 1 else 0.0
    if snr43:
        est = 0.9 * refs[0] + 0.001 * r.standard_normal((C, L)) - 0.02
    else:
        est = 0.8 * refs[0] + 0.07 * second + 0.03 * r.standard_normal((C, L)) - 0.02
    return refs.astype(np.float32), est.astype(np.float32), mix.astype(np.float32)


def plan_windows(L, tile, window=1, hop=1):
    """[(t0, t1)] per window, as the issue defines them (restated here, not imported)"""
    J = -(-L // tile)
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    return [(min(m * hop * tile, L), min((m * hop + window) * tile, L)) for m in range(M)]


def _signals(refs, est, mix, c, C, t0, t1, centre=True):
    f = lambda a: np.asarray(a[..., t0:t1], np.float64)   # noqa: E731
    rc, ec, mx = f(refs[:, c]), f(est[c]), f(mix)
    if centre:
        rc, ec, mx = rc - rc.mean(axis=-1, keepdims=True), ec - ec.mean(), mx - mx.mean(axis=-1, keepdims=True)
    base = mx.mean(axis=0) if C == 1 else mx[c]
    return rc, ec, base


def score_window_direct(refs, est, mix, c, target, t0, t1):
    """The eleven numbers of one window of channel c, float64, straight from the samples."""
    C = refs.shape[1]
    n = t1 - t0
    if n < 2:
        return np.full(11, np.nan)
    rc, ec, base = _signals(refs, est, mix, c, C, t0, t1)
    energy = (rc ** 2).sum(axis=-1)
    if energy[target] == 0:
        return np.full(11, np.nan)
    kept = [i for i in range(rc.shape[0]) if energy[i] != 0]          # a silent source is left out of the projection
    R_ = rc[kept].T
    idx = kept.index(target)
    out = []
    with np.errstate(all="ignore"):
        for x in (ec, base):
            try:
                out.append(O.np_scale_bss_eval_helper(R_, x, idx))
            except np.linalg.LinAlgError:
                out.append(O.np_scale_bss_eval_helper(R_, x, idx, compute_sir_sar=False))
        e, b = out
        return np.array([e[0], e[1], e[2], e[3], e[4], e[5], e[0] - b[0], e[3] - b[3], e[4] - b[4], e[1] - b[1], e[2] - b[2]], np.float64)


def score_direct_f64(refs, est, mix, target=0, tile=16000, window=1, hop=1):
    """One recording: refs [S, C, L], est [C, L], mix [2, L] -> (whole [C, 11], track [C, M, 11])."""
    C, L = refs.shape[1], refs.shape[2]
    wins = plan_windows(L, tile, window, hop)
    whole = np.stack([score_window_direct(refs, est, mix, c, target, 0, L) for c in range(C)])
    track = np.stack([np.stack([score_window_direct(refs, est, mix, c, target, t0, t1) for t0, t1 in wins]) for c in range(C)])
    return whole, track


def gram_rows(refs, est, mix, c, t0, t1, dtype=np.float64):
    """[N] signals of channel c over [t0, t1) in the kernel's order: s_0 .. s_{S-1}, est_c, mix_l, mix_r"""
    return [np.asarray(a[t0:t1], dtype) for a in list(refs[:, c]) + [est[c], mix[0], mix[1]]]


def gram_f64(rows, dtype=np.float64):
    """Sums and Gram matrix of `rows` in m2h_score_gram's layout: [N + N(N+1)/2]."""
    N = len(rows)
    return np.array([a.sum(dtype=dtype) for a in rows] + [(rows[i] * rows[k]).sum(dtype=dtype) for i in range(N) for k in range(i, N)], dtype)


def gram_abs(rows):
    """sum |a| and sum |a b| in the same layout (the scale of the element-wise bound), float64"""
    N = len(rows)
    rows = [np.abs(np.asarray(a, np.float64)) for a in rows]
    return np.array([a.sum() for a in rows] + [(rows[i] * rows[k]).sum() for i in range(N) for k in range(i, N)])


def gram_recording(refs, est, mix, windows):
    """[C, len(windows), K] float64 Gram rows of one recording"""
    C = refs.shape[1]
    return np.stack([np.stack([gram_f64(gram_rows(refs, est, mix, c, t0, t1)) for t0, t1 in windows]) for c in range(C)])


def max_err(got, want, cols=ALL):
    """Largest |got - want| over `cols` in dB; equal infinities and NaN in the same place count as 0, a NaN or infinity on one side only as inf."""
    got, want = np.asarray(got, np.float64)[..., list(cols)], np.asarray(want, np.float64)[..., list(cols)]
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & (got == want))
    with np.errstate(all="ignore"):
        d = np.where(same, 0.0, np.abs(got - want))
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0
