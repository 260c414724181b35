"""The Scorer's BSS-eval numbers (m2h/audio/score.py, "BSS") restated in numpy float64: SDR, SIR and SAR of one target through a
time-invariant distortion filter of T taps (bss_eval_sources for one target without permutation search, one filter set from the whole
recording, window numbers from that filter's components), of the estimate and of the mixture as baseline, and the three improvements.
Shared by tests/test_score_bss_cpu.py and tests/test_gpu_score_bss.py; no GPU, no m2h import.

The definition is written twice, independently: route "a" takes the correlations from a power-of-two FFT, solves by LU (np.linalg.solve)
and filters with np.convolve; route "b" takes them from a transform of 3 * 2^k points, solves by Cholesky and filters with
scipy.signal.fftconvolve.  explicit_gram() builds the Gram matrix of the shifted references sample by sample, for small T.

Bounds of the two kernels (u = 2^-53, gamma_k = k u / (1 - k u); Higham, Accuracy and Stability of Numerical Algorithms, 3.1):
  corr_bound     a sum of n exact products added in any order misses the true sum by at most gamma_{n-1} sum |a b| <= n u sum |a b|.
  project_bound  a filtered sample, K = (taps x signals) fused multiply-adds in any order, misses by eps <= gamma_K sum |h| |s|; a
                 difference of two such values adds u |d|; a sum of m squares of values e known to within eps misses by at most
                 sum (2 |e| eps + eps^2) (1 + gamma_{m+1}) + gamma_{m+1} sum e^2.  The numpy reference obeys the same bound, so the
                 kernel is held to twice it.
"""
import numpy as np

BSS_ORDER = ("sdr", "sir", "sar", "sdr_base", "sir_base", "sar_base", "sdri", "siri", "sari")
# (L, tile, T, S, C)
CASES = ((40, 7, 8, 3, 2), (8, 7, 2, 3, 1), (16001, 16000, 512, 3, 2), (40001, 16000, 512, 3, 1), (40001, 16000, 512, 1, 2),
         (2000, 16000, 512, 3, 1), (4001, 16000, 512, 6, 2))
SPREAD_BSS = 2e-12                # dB: the worst |route a - route b| over CASES, both estimates, whole and track: 1.33e-12 measured, rounded up
TOL_BSS = 64 * SPREAD_BSS         # dB: the GPU against route a.  64 x: a tile-ordered fp64 sum differs more from an FFT sum than two numpy routes do
U = 2.0 ** -53
MUTANTS = ("tail", "lag_sign", "st_joint", "taps", "means", "border", "fp32corr", "base_filters", "nolag")


def gamma(k):
    return k * U / (1.0 - k * U)


def plan(Lr, tile, window=1, hop=1):
    """-> (J, [(j0, j1)] per window), as the issue defines tiles and windows (restated here, not imported)"""
    J = -(-Lr // tile)
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    return J, [(min(m * hop, J), min(m * hop + window, J)) for m in range(M)]


def owned(j0, j1, J, Lr, tile, T):
    """the output samples [n0, n1) of the tiles [j0, j1): tile j owns [j tile, (j + 1) tile) of [0, Lr), the last tile also the tail"""
    if j0 >= j1:
        return 0, 0
    return j0 * tile, (Lr + T - 1 if j1 == J else j1 * tile)


def filtered_estimate(refs, mix, seed):
    """The defect case: the target (reference 0) through a 200-tap decaying FIR with 37 samples of delay, plus a filtered
    interferer and noise -> est [C, L] fp32"""
    S, C, L = refs.shape
    r = np.random.default_rng(seed)
    fir = np.zeros(237)
    fir[37:] = r.standard_normal(200) * np.exp(-np.arange(200) / 40.0)
    fir[37] = 1.0
    fir2 = 0.1 * r.standard_normal(50) * np.exp(-np.arange(50) / 10.0)
    est = []
    for c in range(C):
        e = np.convolve(refs[0, c].astype(np.float64), fir)[:L]
        if S > 1:
            e = e + np.convolve(refs[1, c].astype(np.float64), fir2)[:L]
        est.append(e + 0.01 * r.standard_normal(L))
    return np.stack(est).astype(np.float32)


def signals(refs, est, mix, c, D=0, lag=0):
    """the raw signals of channel c over the region [D, L - D): s [S, Lr], x [Lr] read `lag` samples later, b [Lr]; float64"""
    C, L = refs.shape[1], refs.shape[2]
    s = refs[:, c, D:L - D].astype(np.float64)
    x = est[c, D + lag:L - D + lag].astype(np.float64)
    b = (np.float32(0.5) * (mix[0, D:L - D] + mix[1, D:L - D])) if C == 1 else mix[c, D:L - D]
    return s, x, np.asarray(b, np.float32).astype(np.float64)


def xcorr(a, v, T, route="a"):
    """c[d + T - 1] = sum_t a[t] v[t + d], d = -(T - 1) .. T - 1, both zero outside their samples"""
    n = max(len(a), len(v)) + T
    k = int(np.ceil(np.log2(n)))
    nfft = 1 << k if route == "a" else 3 << max(k - 1, 0)
    cc = np.fft.irfft(np.conj(np.fft.rfft(a, nfft)) * np.fft.rfft(v, nfft), nfft)
    return np.concatenate([cc[nfft - (T - 1):], cc[:T]])


def xcorr_tiles(a, v, T, tile):
    """the `border` defect: every tile correlated on its own samples only"""
    out = np.zeros(2 * T - 1)
    for t0 in range(0, len(a), tile):
        out += xcorr(a[t0:t0 + tile], v[t0:t0 + tile], T)
    return out


def gram_from_lags(c, T):
    """c [S, S, 2 T - 1] -> G [S T, S T]: G[(i, a), (k, b)] = c_ik[a - b]"""
    S = c.shape[0]
    idx = (T - 1) + np.arange(T)[:, None] - np.arange(T)[None, :]
    return c[:, :, idx].transpose(0, 2, 1, 3).reshape(S * T, S * T)


def explicit_gram(s, T):
    """the Gram matrix of the shifted references, sample by sample: Z[(i, a), n] = s_i[n - a], n = 0 .. Lr + T - 2; G = Z Z^T"""
    S, Lr = s.shape
    Z = np.zeros((S, T, Lr + T - 1))
    for a in range(T):
        Z[:, a, a:a + Lr] = s
    Z = Z.reshape(S * T, -1)
    return Z @ Z.T


def lags(s, T, route="a", mutant=None, tile=None):
    """c [S, S, 2 T - 1] of the references"""
    S = s.shape[0]
    c = np.zeros((S, S, 2 * T - 1))
    for i in range(S):
        for k in range(i, S):
            c[i, k] = xcorr_tiles(s[i], s[k], T, tile) if mutant == "border" else xcorr(s[i], s[k], T, route)
            c[k, i] = c[i, k][::-1]
    if mutant == "lag_sign":
        c = c[:, :, ::-1].copy()
    if mutant == "fp32corr":
        c = c.astype(np.float32).astype(np.float64)
    return c


def solve_filters(s, ys, j, T, route="a", mutant=None, tile=None):
    """-> (h [len(ys), S, T] joint, g [len(ys), T] target alone, silent [S] bool); raises np.linalg.LinAlgError when a factorisation fails"""
    S = s.shape[0]
    c = lags(s, T, route, mutant, tile)
    p = []
    for y in ys:
        rows = [(xcorr_tiles(s[i], y, T, tile) if mutant == "border" else xcorr(s[i], y, T, route))[T - 1:] for i in range(S)]
        p.append(np.stack(rows))
    p = np.stack(p)                                                                       # [Y, S, T]
    if mutant == "fp32corr":
        p = p.astype(np.float32).astype(np.float64)
    silent = np.array([c[i, i, T - 1] == 0 for i in range(S)])
    G = gram_from_lags(c, T).reshape(S, T, S, T).copy()
    for i in np.nonzero(silent)[0]:                                                      # left out: identity block, right-hand side 0
        G[i], G[:, :, i] = 0.0, 0.0
        G[i, :, i, :] = np.eye(T)
        p[:, i] = 0.0
    G = G.reshape(S * T, S * T)
    Gj = gram_from_lags(c[j:j + 1, j:j + 1], T)
    rhs, rhs_j = p.reshape(len(ys), S * T).T, p[:, j].T
    if route == "a":
        h, g = np.linalg.solve(G, rhs), np.linalg.solve(Gj, rhs_j)
    else:
        from scipy.linalg import cho_factor, cho_solve
        h, g = cho_solve(cho_factor(G, lower=True), rhs), cho_solve(cho_factor(Gj, lower=True), rhs_j)
    return h.T.reshape(len(ys), S, T), g.T, silent


def components(s, y, h, g, j, route="a"):
    """-> (s_t, P, y zero-extended), each Lr + T - 1 samples"""
    if route == "a":
        conv = np.convolve
    else:
        from scipy.signal import fftconvolve as conv
    st = conv(s[j], g)
    P = sum(conv(s[i], h[i]) for i in range(s.shape[0]))
    return st, P, np.concatenate([y, np.zeros(len(st) - len(y))])


def five_sums(st, P, y, n0, n1):
    st, P, y = st[n0:n1], P[n0:n1], y[n0:n1]
    return np.array([(st ** 2).sum(), ((y - st) ** 2).sum(), ((P - st) ** 2).sum(), (P ** 2).sum(), ((y - P) ** 2).sum()])


def nine(sums):
    """sums [..., 10] -> [..., 9] in BSS_ORDER; IEEE rules"""
    sums = np.asarray(sums, np.float64)
    with np.errstate(all="ignore"):
        e = [10 * np.log10(sums[..., q + 0] / sums[..., q + 1]) for q in (0, 5)], [10 * np.log10(sums[..., q + 0] / sums[..., q + 2]) for q in (0, 5)], \
            [10 * np.log10(sums[..., q + 3] / sums[..., q + 4]) for q in (0, 5)]
        (sdr, sdrb), (sir, sirb), (sar, sarb) = e
        return np.stack([sdr, sir, sar, sdrb, sirb, sarb, sdr - sdrb, sir - sirb, sar - sarb], axis=-1)


def channel_sums(refs, est, mix, c, target, tile, window, hop, T, D=0, lag=0, route="a", mutant=None):
    """one channel -> sums [1 + M, 10]: the whole recording, then every window; NaN rows for a silent target or a failed factorisation.
    With hop=None, `window` is a list of (window, hop) pairs and a list of such arrays comes back, all from one solve."""
    configs = [(window, hop)] if hop is not None else list(window)
    Teff = T - 1 if mutant == "taps" else T
    s, x, b = signals(refs, est, mix, c, D, 0 if mutant == "nolag" else lag)
    if mutant == "means":
        s, x, b = s - s.mean(axis=1, keepdims=True), x - x.mean(), b - b.mean()
    Lr = s.shape[1]
    J = plan(Lr, tile)[0]
    rows = [[(0, J)] + plan(Lr, tile, w, h_)[1] for w, h_ in configs]
    outs = [np.full((len(r), 10), np.nan) for r in rows]
    parts = None
    if (s[target] ** 2).sum() != 0:
        try:
            h, g, _ = solve_filters(s, (x, b), target, Teff, route, mutant, tile)
            if mutant == "base_filters":
                h[1], g[1] = h[0], g[0]
            parts = [components(s, y, h[q], h[q][target] if mutant == "st_joint" else g[q], target, route) for q, y in enumerate((x, b))]
        except np.linalg.LinAlgError:
            pass
    if parts is not None:
        for out, r in zip(outs, rows):
            for q, (st, P, yz) in enumerate(parts):
                for m, (j0, j1) in enumerate(r):
                    n0, n1 = owned(j0, j1, J, Lr, tile, Teff)
                    if mutant == "tail":
                        n1 = min(n1, Lr)
                    out[m, 5 * q:5 * q + 5] = five_sums(st, P, yz, n0, n1)
    return outs[0] if hop is not None else outs


def bss_direct(refs, est, mix, target=0, tile=16000, window=1, hop=1, T=512, D=0, lags_=None, route="a", mutant=None):
    """One recording: refs [S, C, L], est [C, L], mix [2, L] -> (whole [C, 9], track [C, M, 9]); lags_ [C] with D > 0.
    With hop=None, `window` is a list of (window, hop) pairs and a list of such results comes back, all from one solve."""
    C = refs.shape[1]
    per = [channel_sums(refs, est, mix, c, target, tile, window, hop, T, D, 0 if lags_ is None else int(lags_[c]), route, mutant) for c in range(C)]
    if hop is not None:
        rows = np.stack([nine(a) for a in per])
        return rows[:, 0], rows[:, 1:]
    out = []
    for k in range(len(per[0])):
        rows = np.stack([nine(a[k]) for a in per])
        out.append((rows[:, 0], rows[:, 1:]))
    return out


def max_err(got, want):
    """Largest |got - want| in dB; equal infinities and NaN in the same place count as 0, a NaN or infinity on one side only as inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & (got == want))
    with np.errstate(all="ignore"):
        d = np.where(same, 0.0, np.abs(got - want))
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0


# ---- the kernels' own outputs, for the element-wise bounds

def corr_tiles_exact(s, vs, T, tile):
    """m2h_bss_corr's output for one (r, c) in extended precision: s [S, Lr] and vs [S + 2, Lr] float64 (fp32 values)
    -> (c [J, S, S + 2, T] longdouble-accurate as float64, sum |a b| [J, S, S + 2, T], the tiles' sample counts [J])"""
    S, Lr = s.shape
    J = -(-Lr // tile)
    out, mag, cnt = np.zeros((J, S, len(vs), T)), np.zeros((J, S, len(vs), T)), np.zeros(J)
    for j in range(J):
        t0, n = j * tile, min(tile, Lr - j * tile)
        cnt[j] = n
        for k, v in enumerate(vs):
            vp = np.concatenate([v[t0:t0 + n + T - 1], np.zeros(max(0, t0 + n + T - 1 - Lr))])
            win = np.lib.stride_tricks.sliding_window_view(vp, n)[:T]                     # [T, n]: win[d, t] = v[t0 + t + d]
            for i in range(S):
                prod = win * s[i, t0:t0 + n]                                              # exact: 24-bit x 24-bit in float64
                out[j, i, k] = prod.sum(axis=1, dtype=np.longdouble)
                mag[j, i, k] = np.abs(prod).sum(axis=1)
    return out, mag, cnt


def project_tiles(s, x, b, h, target, tile):
    """m2h_bss_project's output for one (r, c) in numpy float64 with the module docstring's bound: s [S, Lr], x, b [Lr],
    h [2, S + 1, T] -> (sums [J, 10], bound [J, 10])"""
    S, Lr = s.shape
    T = h.shape[2]
    J = -(-Lr // tile)
    sums, bound = np.zeros((J, 10)), np.zeros((J, 10))
    for q, y in enumerate((x, b)):
        st, P, yz = components(s, y, h[q, :S], h[q, S], target)
        e_st = gamma(T) * np.convolve(np.abs(s[target]), np.abs(h[q, S]))
        e_P = gamma(S * T) * sum(np.convolve(np.abs(s[i]), np.abs(h[q, i])) for i in range(S))
        vals = (st, yz - st, P - st, P, yz - P)
        errs = (e_st, e_st + U * np.abs(yz - st), e_st + e_P + U * np.abs(P - st), e_P, e_P + U * np.abs(yz - P))
        for j in range(J):
            n0, n1 = owned(j, j + 1, J, Lr, tile, T)
            g = gamma(n1 - n0 + 1)
            for k, (v, e) in enumerate(zip(vals, errs)):
                v, e = v[n0:n1], e[n0:n1]
                sums[j, 5 * q + k] = (v ** 2).sum()
                bound[j, 5 * q + k] = (2 * np.abs(v) * e + e ** 2).sum() * (1 + g) + g * (v ** 2).sum()
    return sums, bound
