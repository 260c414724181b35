"""float64 restatements of m2h.audio.render (the Auralizer) and the inputs of its tests.

render_f64             : the definition, literally -- scipy.signal.fftconvolve per block and ear in float64, placed at jB, summed, then
                         the gained sum over the sources.
render_partitioned_f64 : the algorithm of csrc/render.hip -- block and partition spectra of 32768 points, frames summed over the
                         partitions in ascending order, two frames over every output sample, computed chunk by chunk from render_plan.
                         With dtype=np.float32 the same algorithm on scipy's single-precision FFT: the arithmetic the bound sits above.
DEFECTS                : four wrong renderers (render_f64 with one thing broken) that the GPU test's bound must reject.
"""
import numpy as np
import scipy.fft
from scipy.signal import fftconvolve

B = 16000
NFFT = 32768

# (S, L, Lr, K, tail): the GPU accuracy cases (R = 2 throughout)
CASES = [
    (1, 1, 1, 1, False),               # shorter than anything
    (2, 15999, 700, 1, True),          # one cut block, with its tail
    (3, 16000, 16000, 1, False),       # exactly one block, one full partition
    (3, 16001, 16001, 1, False),       # one-sample second block and one-tap second partition
    (2, 40001, 16001, 3, False),       # moving listener, odd length (unaligned stores), two partitions
    (3, 40001, 33000, 1, True),        # three partitions, frames outnumber blocks
    (3, 40001, 33000, 1, False),
    (3, 40001, 33000, 3, True),
    (3, 40001, 33000, 3, False),
]
R = 2
REL_L1_BOUND = 2e-5                    # the project's bound for fp32 glue against float64 (test_gpu_separate.py, test_gpu_resample.py)
PRODUCT_BOUND = 2e-6 * np.sqrt(15.0)   # m2h_fftconv_full's bound per product, relative to the product's max-abs (test_gpu_feeder.py)


def case_id(c):
    return "S%d-L%d-Lr%d-K%d-%s" % (c[0], c[1], c[2], c[3], "tail" if c[4] else "cut")


def make_sources(R, S, L, seed):
    """noise, sigma 0.1"""
    return (0.1 * np.random.default_rng(seed).standard_normal((R, S, L))).astype(np.float32)


def make_rirs(R, S, K, Lr, seed):
    """noise under an exponential envelope that falls to 1/30 at the last tap: the last partition is never negligible"""
    env = np.exp(-np.log(30.0) * np.arange(Lr) / max(Lr - 1, 1))
    return (np.random.default_rng(seed + 1000).standard_normal((R, S, K, Lr, 2)) * env[None, None, None, :, None]).astype(np.float32)


def make_case(case, seed=0):
    S, L, Lr, K, _ = case
    return make_sources(R, S, L, seed + 7 * L + Lr), make_rirs(R, S, K, Lr, seed + 7 * L + Lr + K)


def default_gains(R, S):
    return np.full((R, S), np.float32(1.0 / S), np.float32)


def rel_l1(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).sum() / np.abs(want).sum())


def mix_f64(images, gains):
    """mix[r, e, n] = sum over s in order of gains[r, s] * image[r, s, e, n]"""
    g = np.asarray(gains, np.float64)
    mix = np.zeros((images.shape[0],) + images.shape[2:], np.float64)
    for s in range(images.shape[1]):
        mix += g[:, s, None, None] * images[:, s]
    return mix


def render_f64(sources, rirs, gains=None, tail=False, defect=None):
    """-> (mix [R, 2, L_out], images [R, S, 2, L_out]) in float64.  defect: one of DEFECTS (a wrong renderer) or None."""
    assert defect is None or defect in DEFECTS
    x, h = np.asarray(sources, np.float64), np.asarray(rirs, np.float64)
    if h.ndim == 4:
        h = h[:, :, None]
    Rn, S, L = x.shape
    K, Lr = h.shape[2], h.shape[3]
    J = -(-L // B)
    assert K in (1, J)
    if defect == "last_partition_dropped":
        h = h[:, :, :, :(-(-Lr // B) - 1) * B]
    L_full = L + Lr - 1
    images = np.zeros((Rn, S, 2, L_full + 1), np.float64)
    for r in range(Rn):
        for s in range(S):
            for j in range(J):
                blk = x[r, s, j * B:min((j + 1) * B, L)]
                k = 0 if K == 1 else j
                if defect == "next_second_rir":
                    k = min(k + 1, K - 1)
                at = j * B + (1 if defect == "blocks_one_sample_late" and j > 0 else 0)
                for e in range(2):
                    y = fftconvolve(blk, h[r, s, k, :, e])
                    if defect == "tail_not_carried":
                        y = y[:B]
                    images[r, s, e, at:at + y.size] += y
    images = images[..., :L_full if tail else L]
    return mix_f64(images, default_gains(Rn, S) if gains is None else gains), images


DEFECTS = ("last_partition_dropped", "blocks_one_sample_late", "next_second_rir", "tail_not_carried")


def product_max(sources, rirs):
    """T: the largest max-abs of any single block x partition convolution, in float64"""
    x, h = np.asarray(sources, np.float64), np.asarray(rirs, np.float64)
    if h.ndim == 4:
        h = h[:, :, None]
    Rn, S, L = x.shape
    K, Lr = h.shape[2], h.shape[3]
    J, Pn = -(-L // B), -(-Lr // B)
    T = 0.0
    for r in range(Rn):
        for s in range(S):
            for j in range(J):
                for p in range(Pn):
                    for e in range(2):
                        T = max(T, np.abs(fftconvolve(x[r, s, j * B:(j + 1) * B], h[r, s, 0 if K == 1 else j, p * B:(p + 1) * B, e])).max())
    return T


def render_partitioned_f64(sources, rirs, gains=None, tail=False, max_blocks=1024, dtype=np.float64):
    """The algorithm of csrc/render.hip -> (mix, images); frames, partition indices and chunks from m2h.audio.render.render_plan."""
    from m2h.audio.render import render_plan
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    x, h = np.asarray(sources, dtype), np.asarray(rirs, dtype)
    if h.ndim == 4:
        h = h[:, :, None]
    Rn, S, L = x.shape
    K, Lr = h.shape[2], h.shape[3]
    plan = render_plan(L, Lr, K, max_blocks, tail)
    J, Pn, F, L_out = plan["J"], plan["Pn"], plan["frames"], plan["L_out"]
    images = np.full((Rn, S, 2, L_out), np.nan, dtype)
    for ch in plan["chunks"]:
        (o0, o1), (m0, m1), (j0, j1), (k0, k1) = ch["out"], ch["frames"], ch["x"], ch["h"]
        X = {j: scipy.fft.rfft(x[:, :, j * B:(j + 1) * B], n=NFFT, axis=-1) for j in range(j0, j1)}                       # [R, S, bins]
        H = {(k, p): scipy.fft.rfft(h[:, :, k, p * B:(p + 1) * B, :], n=NFFT, axis=-2) for k in range(k0, k1) for p in range(Pn)}   # [R, S, bins, 2]
        frames = {}
        for m in range(m0, m1):
            acc = np.zeros((Rn, S, NFFT // 2 + 1, 2), cdtype)
            for p in range(Pn):
                j = m - p
                if 0 <= j < J:
                    acc = acc + X[j][..., None] * H[(0 if K == 1 else j, p)]      # KeyError if the chunk does not hold what the frame reads
            frames[m] = scipy.fft.irfft(acc, n=NFFT, axis=-2)                    # [R, S, NFFT, 2]
            assert frames[m].dtype == dtype
        for o in range(o0, o1):
            n0, n1 = o * B, min((o + 1) * B, L_out)
            v = np.zeros((Rn, S, n1 - n0, 2), dtype)
            if o < F:
                v = v + frames[o][:, :, :n1 - n0]
            if o >= 1:
                v = v + frames[o - 1][:, :, B:B + n1 - n0]
            images[:, :, :, n0:n1] = np.moveaxis(v, -1, -2)
    assert not np.isnan(images).any()                                             # every output block written
    g = default_gains(Rn, S) if gains is None else gains
    if dtype == np.float64:
        return mix_f64(images, g), images
    mix = np.zeros((Rn, 2, L_out), dtype)
    for s in range(S):
        mix = mix + np.asarray(g, dtype)[:, s, None, None] * images[:, s]
    return mix, images
