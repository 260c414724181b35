"""The Scorer's STOI and ESTOI (m2h/audio/score.py, "STOI"), restated in numpy float64 straight from the definition, with a float32
restatement (float32 resampling, windowing and transform; float64 from |S|^2 on) that gives the tolerances the GPU is held to and carries
the planted defects of the mutant table.  Shared by tests/test_score_stoi_cpu.py and tests/test_gpu_score_stoi.py; no GPU, no m2h import.

Definition.  FS = 10000, frames of 256 every 128, NFFT = 512, 15 third-octave bands, segments of 30 frames, BETA = -15 dB (clip factor
1 + 10^0.75), dynamic range 40 dB, EPS = 2^-52, w = hanning(258)[1:-1].  The three signals (clean x, estimate y, baseline b) are
converted from 16 kHz to 10 kHz by the project's resampler definition (tests/resample_ref.py: up / down = 5 / 8).  A range of n samples:
  1. frames at i = 0, 128, ... < n - 256 (exclusive end); e_f = 20 log10(|w x_f| + EPS) from the clean signal; kept iff e_f > max - 40;
     the K kept frames of every signal are windowed and overlap-added at hop 128;
  2. framed again by the same rule (K - 1 frames), windowed again, 512-point transform, X[j, t] = sqrt(sum of |S|^2 over band j's bins);
  3. for m = 30 .. K - 1, the 15 x 30 blocks of columns [m - 30, m): STOI d_m = sum (X^ Y'^) / 15 with alpha = |X_row| / (|Y_row| + EPS),
     Y' = min(alpha Y, (1 + 10^0.75) X), rows centred and divided by (norm + EPS); ESTOI d_m = sum (X~ Y~) / 30 with rows, then columns,
     centred and divided by (norm + EPS); the means of d_m over the segments.
Fewer than 30 envelope frames, or a clean signal whose largest frame energy is 0, give NaN.

Every test input keeps a MASK MARGIN min_f |e_f - (max - 40)| of at least 1 dB in every range (asserted by analyse_recording about its
own inputs), so a kept-frame mismatch can never be excused as rounding.

Sums over the 30 columns of a row and the 15 bands of a column are written as explicit loops in column / band order: the order is then
part of the statement and the same in float64 and longdouble."""
import numpy as np

import resample_ref
from elem_bound import TAU_FP32

FS, FRAME, HOP, NFFT, BANDS, SEG = 10000, 256, 128, 512, 15, 30
EPS = 2.0 ** -52
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
RANGE_DB = 40.0
ORDER = ("stoi", "estoi", "stoi_base", "estoi_base", "stoii", "estoii")
EDGES = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
MIN_MARGIN_DB = 1.0
DEFECTS = ("mask_from_y", "inclusive_frames", "edges_one_late", "clip_without_one", "no_clip", "mean_before_clip", "estoi_columns_first",
           "segment_hop_30", "no_second_window", "no_lag")
# 8 x the worst |float32 restatement - float64| of the six numbers over LENGTHS and the two extra inputs (test_score_stoi_cpu.py measures it
# and holds this constant to it): what the GPU's numbers are held to end to end.  The factor 8 is for another summation order.
TOL_END_TO_END = 2.3e-7
LENGTHS = (16000, 16001, 40001)
SHORT = (6000, 6560, 7000)

W = np.hanning(FRAME + 2)[1:-1]
W32 = W.astype(np.float32)
_UP, _DOWN, _HALF, _TAPS = resample_ref.taps(16000, FS)


def band_edges():
    """the half-open bin ranges of the 15 bands from the formula: the bins nearest to 150 2^((2 j -+ 1) / 6) Hz"""
    f = np.arange(NFFT // 2 + 1) * FS / NFFT
    out = []
    for j in range(BANDS):
        lo, hi = 150.0 * 2.0 ** ((2 * j - 1) / 6.0), 150.0 * 2.0 ** ((2 * j + 1) / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return out


def resample(x, f32=False):
    """[..., L] at 16 kHz -> [..., ceil(5 L / 8)] at 10 kHz, float64; f32: the float32 table and a float32 chain k = 0 .. T - 1"""
    x = np.asarray(x)
    lead = x.shape[:-1]
    rows = x.reshape(-1, x.shape[-1])
    if not f32:
        return resample_ref.polyphase(rows, _TAPS, _UP, _DOWN, _HALF).reshape(lead + (-1,))
    L = rows.shape[1]
    T = -(-len(_TAPS) // _UP)
    hp = np.zeros(T * _UP, np.float32)
    hp[:len(_TAPS)] = _TAPS.astype(np.float32)
    G = hp.reshape(T, _UP).T
    n = np.arange(resample_ref.out_len(L, _UP, _DOWN), dtype=np.int64)
    t = n * _DOWN + _HALF
    p, j0 = t % _UP, t // _UP
    acc = np.zeros((rows.shape[0], len(n)), np.float32)
    r32 = rows.astype(np.float32)
    for k in range(T):
        j = j0 - k
        ok = (j >= 0) & (j < L)
        v = np.where(ok, r32[:, np.clip(j, 0, L - 1)], np.float32(0))
        acc = (G[p, k].astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)     # one rounding per step, as fmaf
    return acc.astype(np.float64).reshape(lead + (-1,))


def frame_starts(n, defect=()):
    return range(0, n - FRAME + (1 if "inclusive_frames" in defect else 0), HOP)


def frame_count(n):
    return len(frame_starts(n))


def _ola(frames):
    """[K, 256] windowed frames -> their overlap-add at hop 128, (K - 1) 128 + 256 samples"""
    K = frames.shape[0]
    out = np.zeros((K - 1) * HOP + FRAME, frames.dtype)
    for k in range(K):
        out[k * HOP:k * HOP + FRAME] += frames[k]
    return out


def _seq_sum(a, axis):
    """the sum along `axis` in index order"""
    a = np.moveaxis(a, axis, 0)
    s = a[0].copy()
    for i in range(1, a.shape[0]):
        s = s + a[i]
    return s


def _normalise(a, axis):
    """mean removed along `axis`, divided by (norm + EPS), both sums in index order"""
    n = a.shape[axis]
    a = a - np.expand_dims(_seq_sum(a, axis) / n, axis)
    return a / (np.expand_dims(np.sqrt(_seq_sum(a * a, axis)), axis) + a.dtype.type(EPS))


def step3(X, Y, defect=(), dtype=np.float64):
    """(STOI, ESTOI) of the envelopes X (clean), Y (processed) [15, T]; NaN for T < 30.  dtype np.longdouble measures this function's own
    rounding."""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    T = X.shape[1]
    if T < SEG:
        return np.nan, np.nan
    ms = range(SEG, T + 1, SEG if "segment_hop_30" in defect else 1)
    xs = np.stack([X[:, m - SEG:m] for m in ms])                                        # [segments, 15, 30]
    ys = np.stack([Y[:, m - SEG:m] for m in ms])
    eps = dtype(EPS)
    alpha = np.sqrt(_seq_sum(xs * xs, 2)) / (np.sqrt(_seq_sum(ys * ys, 2)) + eps)
    ay = ys * alpha[:, :, None]
    clip = dtype(CLIP) - (1 if "clip_without_one" in defect else 0)
    if "mean_before_clip" in defect:
        ay = ay - (_seq_sum(ay, 2) / SEG)[:, :, None]
    yp = ay if "no_clip" in defect else np.minimum(ay, xs * clip)
    d = _seq_sum(_seq_sum(_normalise(xs, 2) * _normalise(yp, 2), 2), 1) / BANDS
    order = (1, 2) if "estoi_columns_first" in defect else (2, 1)
    xe, ye = xs, ys
    for axis in order:
        xe, ye = _normalise(xe, axis), _normalise(ye, axis)
    de = _seq_sum(_seq_sum(xe * ye, 2), 1) / SEG
    return float(_seq_sum(d, 0) / len(d)), float(_seq_sum(de, 0) / len(de))


def analyse(x, ys, f32=False, defect=()):
    """One range: x the clean signal and ys the processed signals (estimate, baseline), 10 kHz float64 of one length ->
    {"mask" [frames] bool, "K", "margin" dB, "silent", "env" [1 + len(ys), 15, K - 1], "unit" [1 + len(ys), K - 1]: the element bound's
    sqrt(2) TAU_FP32 |frame w|_2 per envelope frame, "stoi"/"estoi": one per processed signal}."""
    sig = [np.asarray(x, np.float64)] + [np.asarray(y, np.float64) for y in ys]
    n = len(sig[0])
    dt = np.float32 if f32 else np.float64
    w = W32 if f32 else W
    starts = list(frame_starts(n, defect))
    nan = [np.nan] * len(ys)
    if not starts:
        return {"mask": np.zeros(0, bool), "K": 0, "margin": np.inf, "silent": False, "env": np.zeros((len(sig), BANDS, 0)),
                "unit": np.zeros((len(sig), 0)), "stoi": nan, "estoi": nan}
    fr = [np.stack([s[i:i + FRAME] for i in starts]).astype(dt) * w for s in sig]      # [frames, 256] windowed
    ref = fr[1] if "mask_from_y" in defect else fr[0]
    norms = np.sqrt((ref.astype(np.float64) ** 2).sum(axis=1))
    with np.errstate(divide="ignore"):
        e = 20.0 * np.log10(norms + EPS)
    mask = e > e.max() - RANGE_DB
    margin = float(np.min(np.abs(e - (e.max() - RANGE_DB))))
    K = int(mask.sum())
    silent = bool(norms.max() == 0)
    out = {"mask": mask, "K": K, "margin": margin, "silent": silent}
    if K < 2:
        out.update({"env": np.zeros((len(sig), BANDS, 0)), "unit": np.zeros((len(sig), 0)), "stoi": nan, "estoi": nan})
        return out
    env, unit = [], []
    for f in fr:
        s = _ola(f[mask])
        fr2 = np.stack([s[i:i + FRAME] for i in frame_starts(len(s), defect)])
        if "no_second_window" not in defect:
            fr2 = fr2 * w
        unit.append(np.sqrt(2.0) * TAU_FP32 * np.sqrt((fr2.astype(np.float64) ** 2).sum(axis=1)))
        if f32:
            re, im = fr2 @ _dft32()[0], fr2 @ _dft32()[1]
            p = re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2               # [frames, 257]
        else:
            p = np.abs(np.fft.rfft(fr2, NFFT, axis=1)) ** 2
        shift = 1 if "edges_one_late" in defect else 0
        env.append(np.stack([np.sqrt(p[:, EDGES[j] + shift:EDGES[j + 1] + shift].sum(axis=1)) for j in range(BANDS)]))
    out["env"], out["unit"] = np.stack(env), np.stack(unit)
    res = [step3(env[0], env[q], defect) if not silent else (np.nan, np.nan) for q in range(1, len(sig))]
    out["stoi"], out["estoi"] = [r[0] for r in res], [r[1] for r in res]
    return out


_dft = []


def _dft32():
    if not _dft:
        ang = 2.0 * np.pi * ((np.arange(FRAME)[:, None] * np.arange(NFFT // 2 + 1)[None, :]) % NFFT) / NFFT
        _dft.extend([np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32)])
    return _dft


def six(a):
    """analyse()'s result for (estimate, baseline) -> the six numbers in ORDER"""
    s, e = a["stoi"], a["estoi"]
    return np.array([s[0], e[0], s[1], e[1], s[0] - s[1], e[0] - e[1]])


def env_bound(a):
    """the element bound of analyse()'s envelopes [signals, 15, K - 1]: every bin moves by at most `unit`, a band's norm by sqrt(bins) unit"""
    nb = np.sqrt(np.diff(np.array(EDGES)).astype(np.float64))
    return a["unit"][:, None, :] * nb[None, :, None]


def worst(got, want, bound):
    """the largest |got - want| / bound; a difference where the bound is 0 counts as inf"""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(all="ignore"):
        q = np.where(d == 0, 0.0, d / bound)
    return float(np.max(q)) if q.size else 0.0


def ranges(Lr, window=1, hop=1):
    """[(start, end)] at 10 kHz for a scored region of Lr samples at 16 kHz: the whole recording, then every window (the plan restated)"""
    L10 = -(-Lr * 5 // 8)
    J = -(-Lr // 16000)
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    return [(0, L10)] + [(min(m * hop * FS, L10), min((m * hop + window) * FS, L10)) for m in range(M)]


def signals16(refs, est, mix, c, target=0, lag=0, D=0, defect=()):
    """one recording: refs [S, C, L], est [C, L], mix [2, L] -> (x, y, b) of channel c at 16 kHz over the region [D, L - D), the estimate
    read `lag` samples later; the mono baseline is formed in float32, as the definition says"""
    L = refs.shape[-1]
    if "no_lag" in defect:
        lag = 0
    x, y = refs[target, c, D:L - D], est[c, D + lag:L - D + lag]
    b = mix[c, D:L - D] if refs.shape[1] == 2 else np.float32(0.5) * (np.asarray(mix[0, D:L - D], np.float32) + np.asarray(mix[1, D:L - D], np.float32))
    return [np.asarray(v, np.float64) for v in (x, y, b)]


def analyse_recording(refs, est, mix, target=0, lag=None, D=0, window=1, hop=1, f32=False, defect=(), check_margin=True):
    """one recording -> {"six": [C, 1 + M, 6], "K": [C, 1 + M], "ranges": [...], "parts": [C][1 + M] analyse() results, "x10": [C, 3, L10]};
    the mask margin of every range is asserted (float64, no defect)."""
    C = refs.shape[1]
    rg = ranges(refs.shape[-1] - 2 * D, window, hop)
    parts, x10s = [], []
    for c in range(C):
        x10 = resample(np.stack(signals16(refs, est, mix, c, target, 0 if lag is None else lag[c], D, defect)), f32)
        x10s.append(x10)
        row = [analyse(x10[0, s:e], [x10[1, s:e], x10[2, s:e]], f32, defect) for s, e in rg]
        if check_margin and not f32 and not defect:
            for (s, e), a in zip(rg, row):
                assert a["margin"] >= MIN_MARGIN_DB, "a test input with a mask margin of %.3f dB in the range [%d, %d)" % (a["margin"], s, e)
        parts.append(row)
    return {"six": np.array([[six(a) for a in row] for row in parts]), "K": np.array([[a["K"] for a in row] for row in parts]), "ranges": rg,
            "parts": parts, "x10": np.stack(x10s)}


def envelope(L, gaps=True):
    t = np.arange(L) / 16000.0
    e = 0.05 + np.abs(np.sin(2.0 * np.pi * 3.0 * t))
    return e * ((t % 0.5) > 0.12) if gaps else e


def inputs(L, seed, S=1, C=1, gaps=True, target=None):
    """-> refs [S, C, L], est [C, L], mix [2, L] float32 and the target index: every source is noise under an envelope
    (0.05 + |sin 2 pi 3 t|) [t mod 0.5 > 0.12] -- real silent gaps, which step 1 removes --, the interferers 0.2 x as loud; with `noise`
    white at 0.3 x the clean signal's peak level, the estimate is clean + 0.3 noise and the mixture is all sources + noise.  The target
    (the loud source) is the last one unless given."""
    r = np.random.default_rng(seed)
    env = envelope(L, gaps)
    target = S - 1 if target is None else target
    gains = np.full(S, 0.2)
    gains[target] = 1.0
    ears = np.array([1.0, 0.8])[:C]
    src = r.standard_normal((S, L)) * env
    refs = gains[:, None, None] * ears[None, :, None] * src[:, None, :]
    noise = 0.3 * r.standard_normal((2, L))
    est = refs[target] + 0.3 * noise[:C]
    mix = refs.sum(axis=0)[[0, C - 1]] + noise
    return refs.astype(np.float32), est.astype(np.float32), mix.astype(np.float32), target


def exclusive_end_length():
    """a 16 kHz length whose 10 kHz length n has n - 256 a multiple of 128: the last full frame is dropped by the exclusive end"""
    n = FRAME + 80 * HOP                                                                 # 10496 samples at 10 kHz: 80 frames, not 81
    L = n * 8 // 5
    assert -(-L * 5 // 8) == n and (n - FRAME) % HOP == 0
    return L


def cases():
    """the inputs the tolerances are measured on: (name, refs, est, mix, target), made once and read-only"""
    if not _cases:
        for L in LENGTHS + (exclusive_end_length(),):
            for S, C in ((1, 1), (3, 2)):
                _cases.append((("gaps", L, S, C),) + inputs(L, 7 + L % 5, S, C))
        _cases.append((("no gaps", 16000, 1, 1),) + inputs(16000, 3, 1, 1, gaps=False))
        for case in _cases:
            for a in case[1:4]:
                a.setflags(write=False)
    return _cases


_cases = []
