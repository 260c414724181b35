"""RoomAcoustics' three kernels path by path (TEST INFRASTRUCTURE): csrc/rir_acoustics.hip rir_onset_kernel, rir_band_energy_kernel and
rir_decay_kernel -- the table of test rows, the cells the rows must reach, the kernels' own searches and scans restated, and named mutants.
tests/acoustics_ref.py keeps the definition (analyze_f64, decay_f64), the scales and band_energy_fp32, which is reused as it is.

tests/test_gpu_acoustics_kernels.py runs every row through m2h_rir_onset, m2h_rir_band_energy and m2h_rir_decay against the definition;
tests/test_acoustics_kernels_cpu.py checks without a GPU that the rows reach every cell, that the restatements stay inside their ceilings on
every row, that every mutant leaves the bound on the rows named for it by MIN_MARGIN at the least, and that the restated constants are the
source's.

Rules (tests/render_kernels.py states them): every element compared, the RIRs inside NaN, every output NaN (-(1 << 30) for the ints) before
the call, onset and peak equal to the definition's, sums / energy / iacf inside |g - r| <= tau s with acoustics_ref's scales.

RIR rows (one RIR each; noise is acoustics_ref.noise_rir or _quiet: enveloped noise of amplitude 0.01, under every planted sample's threshold):
  late      late.lead4000 (Lr 16000: two segments, segment 1 past the row: the zero-fill branch), late.lead20000 (Lr 30001: segments 1 and 2),
            late.last_sample (all zeros but h[15999] = (1, -0.5): n0 = Lr - 1)
  search    pre_echo (a right-ear -0.2 at 60 before a left direct sound of -1 at 100: the onset is the right ear's, the peak is not the onset,
            the peak is negative), tie.same_thread (-1 and +1 at 100 and 2148 = 100 + 2 x 1024), tie.higher_thread (1000 and 1030: thread 1000
            holds the earlier index, thread 6 the later), tie.tree (1001 and 1032, see below), tie.adjacent (100 and 101), peak_near_end (9 samples before the row's end: the direct
            window is cut), threshold (a sample v at 50 before a direct sound pk at 100 with v >= 0.1f * pk in float32 and v < 0.1 * (double)pk:
            threshold_pair() searches them with a fixed seed)
  borders   Lr = 12256 (one whole segment), 12257 (a second segment of one sample), 24512, 17, 16, and 900 with a lead of 200 (the 1280-sample
            IACF window runs past the row)
Decay rows (bins of the test's making): nb in {1, 63, 64, 65, 128, 129, 16000} x rows in {1, 4, 5}; zero_tail (nb 300, the last 70 bins zero: a
whole chunk of zeros and a partial one); one_bin (the -5 .. -25 dB range holds exactly one bin: t20 is NaN).

Kinds and taus.  The RIR rows are a kind of their own: RESTATEMENT_WORST here is the ceiling the CPU test holds the restatements under on
THESE rows, TAU = 8 x that; acoustics_ref's ceilings stay as they are for its cases.  Measured on these rows: energy 4.10e-7 (Lr24512), iacf
3.17e-7 (tie.tree), drr sums 4.42e-16 (tie.tree: two ulps of the order of summation).  The issue's 6.2e-7 and 3.3e-7 came from rows of
other seeds; with these the energy and iacf ceilings come out as acoustics_ref's own (5.0e-7, 3.2e-7: no wider), and only the drr sums need a
higher one (5.0e-16 against 3.3e-16).  The decay rows follow acoustics_ref's rule, 100 x DECAY_ULP_CHANGE; the restated scan is held to an
eighth of that (measured 7.1e-15 at the worst, nb65.rows5).

+ tie.tree, a row beyond the issue's: the tree compares slot t with slot t + o, and two threads meet at the lowest bit in which their numbers
differ; the one whose bit is 0 is "a", and a tree that ignores the index keeps a.  Threads 1000 and 6 (tie.higher_thread) meet at bit 1, where
thread 1000 -- the earlier index -- is a: that mutant is right there by chance.  Threads 1001 and 8 (samples 1001 and 1032) meet at bit 0 with
the later index as a: the mutant is named for this row.

The zero-fill mutant "taken one segment early" cannot show on the late rows (their last live segment is segment 0, which the branch exempts):
it is named for the rows whose last segment g >= 1 is live, Lr24512 and Lr12257.
"""
import numpy as np

import acoustics_ref as R

F32 = np.float32
MIN_MARGIN = 4.0
THREADS, DECAY_ROWS, DECAY_CHUNK = 1024, 4, 64
PAD = 1000
INT_FILL = -(1 << 30)

RESTATEMENT_WORST = {"energy": 5.0e-7, "iacf": 3.2e-7, "drr_sums": 5.0e-16}      # measured 4.10e-7, 3.17e-7, 4.42e-16 on RIR_ROWS (the CPU test pins them)
TAU = {k: 8 * v for k, v in RESTATEMENT_WORST.items()}
DECAY_BOUND = 100 * R.DECAY_ULP_CHANGE
DECAY_RESTATEMENT_WORST = DECAY_BOUND / 8

ONSET_MUTANTS = ("a thread's tie takes the later index", "the tree ignores the index on ties", "threshold in float32", "onset from the left ear only",
                 "direct window not clipped at the row's end")
ENERGY_MUTANTS = ("zero-fill branch writes nothing", "zero-fill branch taken one segment early")
DECAY_MUTANTS = ("carry dropped at a chunk border", "last partial chunk reads past nb")


# ----------------------------------------------------------------------------------------------------------------------------------
# RIR rows
# ----------------------------------------------------------------------------------------------------------------------------------
def _quiet(Lr, seed, T60=0.1):
    g = np.random.default_rng(seed)
    env = 10.0 ** (-3.0 * np.arange(Lr, dtype=np.float64) / (T60 * R.RATE))
    return 0.01 * g.standard_normal((Lr, 2)) * env[:, None]


def threshold_pair(seed=7):
    """(pk, v) float32 with v >= 0.1f * pk in float32 and v < 0.1 * (double)pk: the first pk of a seeded draw with fl(0.1f pk) < 0.1 pk"""
    g = np.random.default_rng(seed)
    for pk in g.uniform(0.5, 1.0, 1000).astype(F32):
        v = F32(0.1) * pk
        assert v.dtype == F32
        if float(v) < 0.1 * float(pk):
            return pk, v
    raise AssertionError("no pair found")


def _planted(Lr, seed, plants):
    h = _quiet(Lr, seed)
    for n, e, v in plants:
        h[n, e] = v
    return h.astype(F32)


def _rir_rows():
    rows = {}
    rows["late.lead4000"] = R.noise_rir(12000, 0.3, 51, lead=4000)
    rows["late.lead20000"] = R.noise_rir(10001, 0.3, 52, lead=20000)
    last = np.zeros((16000, 2), dtype=F32)
    last[15999] = (1.0, -0.5)
    rows["late.last_sample"] = last
    pre = -R.noise_rir(2900, 0.1, 53, lead=100)
    pre[60, 1] = -0.2
    rows["pre_echo"] = pre
    rows["tie.same_thread"] = _planted(3000, 54, [(100, 0, -1.0), (2148, 0, 1.0), (105, 1, -0.5), (2153, 1, 0.5)])
    rows["tie.higher_thread"] = _planted(3000, 55, [(1000, 0, 1.0), (1030, 0, -1.0), (1000, 1, 0.5), (1030, 1, 0.5)])
    rows["tie.tree"] = _planted(3000, 61, [(1001, 0, 1.0), (1032, 0, -1.0), (1001, 1, 0.5), (1032, 1, 0.5)])
    rows["tie.adjacent"] = _planted(3000, 56, [(100, 0, 1.0), (101, 0, 1.0), (103, 1, -0.5), (104, 1, -0.5)])
    rows["peak_near_end"] = _planted(3000, 57, [(2990, 0, 1.0), (2990, 1, 0.7)])
    pk, v = threshold_pair()
    rows["threshold"] = _planted(3000, 58, [(50, 0, v), (100, 0, pk), (100, 1, F32(0.5) * pk)])
    for Lr, T in ((12256, 0.3), (12257, 0.3), (24512, 0.6), (17, 0.05), (16, 0.05)):
        rows["Lr%d" % Lr] = R.noise_rir(Lr, T, 60 + Lr % 50)
    rows["Lr900.lead200"] = R.noise_rir(700, 0.05, 59, lead=200)
    return rows


RIR_ROWS = _rir_rows()
_REF = {}


def reference(name):
    """acoustics_ref.analyze_f64 of a row, computed once"""
    if name not in _REF:
        _REF[name] = R.analyze_f64(RIR_ROWS[name])
    return _REF[name]


def zero_filled_segments(n0, Lr):
    """the segments g > 0 whose bins lie past the row, and the number of segments"""
    nbs = -(-Lr // R.BIN)
    segs = -(-nbs // R.SEG_BINS)
    return [g for g in range(1, segs) if n0 + R.HOP * g >= Lr], segs


def rir_cells(name):
    h, ref = RIR_ROWS[name], reference(name)
    Lr = h.shape[0]
    n0, npk = ref["onset"], [int(v) for v in ref["peak"]]
    out = set()
    zf, segs = zero_filled_segments(n0, Lr)
    out.add("segments: %d" % min(segs, 3))
    if zf:
        out.add("zero-fill branch")
    if len(zf) > 1:
        out.add("zero-fill branch, two segments")
    if zf and len(zf) < segs - 1:
        out.add("a live segment g > 0 before a zero-filled one")
    if segs > 1 and not zf:
        out.add("every segment g > 0 live")
    mag = np.abs(h.astype(np.float64))
    pk = mag.max(0)
    firsts = [int(np.argmax(mag[:, e] >= 0.1 * pk[e])) if pk[e] > 0 else Lr for e in range(2)]
    if firsts[1] < firsts[0]:
        out.add("onset ear = right")
    if npk[0] != n0 and npk[1] != n0:
        out.add("peak != onset")
    for e in range(2):
        at = np.nonzero(mag[:, e] == pk[e])[0]
        if h[npk[e], e] < 0:
            out.add("negative peak")
        if len(at) > 1:
            a, b = int(at[0]), int(at[1])
            out.add("tie: same thread" if a % THREADS == b % THREADS else "tie: adjacent threads" if b == a + 1 else
                    "tie: the earlier index in the higher thread" if a % THREADS > b % THREADS else "tie: the earlier index in the lower thread")
        if npk[e] + R.DIRECT >= Lr:
            out.add("direct window cut at the row's end")
        if npk[e] - R.DIRECT < 0:
            out.add("direct window cut at the row's start")
        v32 = np.abs(h[:, e])
        if pk[e] > 0 and ((v32 >= F32(0.1) * F32(pk[e])) != (mag[:, e] >= 0.1 * pk[e])).any():
            out.add("threshold: float32 and float64 disagree")
    if n0 == Lr - 1:
        out.add("n0 = Lr - 1")
    if n0 > 0:
        out.add("n0 > 0")
    if n0 + R.WIN > Lr:
        out.add("IACF window past the row")
    out.add("Lr % 16 = 0" if Lr % R.BIN == 0 else "Lr % 16 != 0")
    if Lr - n0 == R.HOP:
        out.add("Lr - n0 = one hop exactly")
    if Lr - n0 == R.HOP + 1:
        out.add("Lr - n0 = one hop + 1")
    if Lr - n0 == 2 * R.HOP:
        out.add("Lr - n0 = two hops exactly")
    if Lr <= 2 * R.MAXLAG + 1:
        out.add("Lr inside the lag range")
    return out


RIR_ALL_CELLS = frozenset((
    "segments: 1", "segments: 2", "segments: 3", "zero-fill branch", "zero-fill branch, two segments", "every segment g > 0 live", "onset ear = right", "peak != onset",
    "negative peak", "tie: same thread", "tie: adjacent threads", "tie: the earlier index in the higher thread", "direct window cut at the row's end",
    "direct window cut at the row's start", "threshold: float32 and float64 disagree", "n0 = Lr - 1", "n0 > 0", "IACF window past the row", "Lr % 16 = 0", "Lr % 16 != 0",
    "Lr - n0 = one hop exactly", "Lr - n0 = one hop + 1", "Lr - n0 = two hops exactly", "Lr inside the lag range"))


# ----------------------------------------------------------------------------------------------------------------------------------
# rir_onset_kernel, restated: the two-level search, the fp64 threshold, min over the ears, the silent-ear rules, the strided sums
# ----------------------------------------------------------------------------------------------------------------------------------
def _tree_sum(v, Lr):
    part = np.zeros(THREADS)
    for k in range(0, Lr, THREADS):
        part[:min(THREADS, Lr - k)] += v[k:k + THREADS]
    while part.size > 1:
        part = part[:part.size // 2] + part[part.size // 2:]
    return part[0]


def onset_search_fp32(h, mutant=None):
    """-> n0, npk [2], sums [2, 2] (D, T per ear): no call of onset_f64.  The row is taken to lie inside NaN, as the GPU test lays it."""
    h32 = np.asarray(h, dtype=F32)
    Lr = h32.shape[0]
    mag = np.abs(h32)
    pke, npk, first = [], [], []
    for e in range(2):
        pk, ix = np.zeros(THREADS, dtype=F32), np.zeros(THREADS, dtype=np.int64)
        for base in range(0, Lr, THREADS):                                  # pass 1: a thread walks n = tid, tid + 1024, ..: the first index of its maximum
            v = mag[base:base + THREADS, e]
            t = np.arange(v.size)
            up = (v >= pk[:v.size]) if mutant == ONSET_MUTANTS[0] else (v > pk[:v.size])
            pk[t[up]], ix[t[up]] = v[up], base + t[up]
        o = THREADS // 2
        while o >= 1:                                                       # the tree: the larger value, on ties the lower index
            a, b, ia, ib = pk[:o], pk[o:2 * o], ix[:o], ix[o:2 * o]
            take = (b > a) if mutant == ONSET_MUTANTS[1] else ((b > a) | ((b == a) & (ib < ia)))
            pk, ix = np.where(take, b, a), np.where(take, ib, ia)
            o //= 2
        pke.append(pk[0])
        npk.append(int(ix[0]) if pk[0] > 0 else 0)
        if mutant == ONSET_MUTANTS[2]:
            hit = mag[:, e] >= F32(0.1) * pk[0]
        else:
            hit = mag[:, e].astype(np.float64) >= 0.1 * float(pk[0])        # pass 2: the threshold in fp64
        first.append(int(np.argmax(hit)) if pk[0] > 0 and hit.any() else Lr)
    n0 = first[0] if mutant == ONSET_MUTANTS[3] else min(first)
    n0 = n0 if n0 < Lr else 0
    sums = np.zeros((2, 2))
    n = np.arange(Lr)
    for e in range(2):
        sq = h32[:, e].astype(np.float64) ** 2
        inside = (n >= npk[e] - R.DIRECT) & (n <= npk[e] + R.DIRECT)
        sums[e, 0], sums[e, 1] = _tree_sum(np.where(inside, sq, 0.0), Lr), _tree_sum(sq, Lr)
        if mutant == ONSET_MUTANTS[4] and npk[e] + R.DIRECT >= Lr:
            sums[e, 0] = np.nan                                             # (the next RIR's samples: NaN in the planted buffer)
    return n0, npk, sums


def band_energy_mutant(h, n0, mutant):
    """acoustics_ref.band_energy_fp32's energy with a mutant of the zero-fill branch; the buffer is NaN before the call"""
    E, iacf = R.band_energy_fp32(h, n0)
    Lr = np.shape(h)[0]
    zf, segs = zero_filled_segments(n0, Lr)
    if mutant == ENERGY_MUTANTS[0]:
        for g in zf:
            E[:, :, R.SEG_BINS * g:R.SEG_BINS * (g + 1)] = np.nan
    if mutant == ENERGY_MUTANTS[1]:
        for g in range(1, segs):
            if n0 + R.HOP * (g + 1) >= Lr:
                E[:, :, R.SEG_BINS * g:R.SEG_BINS * (g + 1)] = 0.0
    return E


ONSET_MUTANT_ROWS = {ONSET_MUTANTS[0]: ("tie.same_thread",), ONSET_MUTANTS[1]: ("tie.tree",), ONSET_MUTANTS[2]: ("threshold",), ONSET_MUTANTS[3]: ("pre_echo",),
                     ONSET_MUTANTS[4]: ("peak_near_end", "late.last_sample")}
ENERGY_MUTANT_ROWS = {ENERGY_MUTANTS[0]: ("late.lead4000", "late.lead20000", "late.last_sample"), ENERGY_MUTANTS[1]: ("Lr24512", "Lr12257")}


# ----------------------------------------------------------------------------------------------------------------------------------
# rir_decay_kernel, restated: the total, the reverse scan in chunks of 64 with its carry, the two runs
# ----------------------------------------------------------------------------------------------------------------------------------
DECAY_NB, DECAY_ROW_COUNTS = (1, 63, 64, 65, 128, 129, 16000), (1, 4, 5)


def _decay_row(nb, seed):
    g = np.random.default_rng(seed)
    T = 8.0 if nb > 1000 else max(nb, 2) / 1000.0 * 0.8
    return 10.0 ** (-6.0 * np.arange(nb) / (T * 1000.0)) * (0.5 + g.random(nb))


def decay_tables():
    """name -> bins [rows, nb] float64"""
    out = {}
    for nb in DECAY_NB:
        for rows in DECAY_ROW_COUNTS:
            out["nb%d.rows%d" % (nb, rows)] = np.stack([_decay_row(nb, 1000 * rows + 7 * r + nb) * (1.0 + r) for r in range(rows)])
    tail = _decay_row(300, 5)
    tail[230:] = 0.0
    out["zero_tail"] = np.stack([tail, 2.0 * tail])
    edc = np.array([1.0, 0.5, 0.05, 1e-4, 1e-5, 0.0])
    out["one_bin"] = (edc[:-1] - edc[1:])[None, :]
    return out


DECAY_TABLES = decay_tables()


def decay_cells(name):
    E = DECAY_TABLES[name]
    rows, nb = E.shape
    out = {"nb % 64 = " + ("0" if nb % 64 == 0 else "1" if nb % 64 == 1 else "63" if nb % 64 == 63 else "other"), "chunks: %s" % (min(-(-nb // 64), 3)),
           "rows % 4 = 0" if rows % DECAY_ROWS == 0 else "rows % 4 != 0", "one workgroup" if rows <= DECAY_ROWS else "two workgroups"}
    if nb == 1:
        out.add("nb = 1")
    z = int((np.cumsum(E[0][::-1]) == 0).sum())
    if z >= DECAY_CHUNK:
        out.add("a whole chunk of zero bins at the end")
    want = np.stack([R.decay_f64(r) for r in E])
    if np.isnan(want[:, 1]).any() and np.isfinite(want[:, 0]).any():
        out.add("a range with one bin: t20 NaN beside a finite edt")
    return out


DECAY_ALL_CELLS = frozenset(("nb % 64 = 0", "nb % 64 = 1", "nb % 64 = 63", "nb % 64 = other", "chunks: 1", "chunks: 2", "chunks: 3", "rows % 4 = 0", "rows % 4 != 0",
                             "one workgroup", "two workgroups", "nb = 1", "a whole chunk of zero bins at the end", "a range with one bin: t20 NaN beside a finite edt"))


def _pairwise64(v):
    """the xor-32 .. 1 exchange sum of 64 lanes"""
    v = np.asarray(v, dtype=np.float64).copy()
    o = 32
    while o >= 1:
        v = v + v[np.arange(64) ^ o]
        o >>= 1
    return v[0]


def _lane_sum(vals, idx):
    """a wave's sum: a lane adds its elements (index % 64) in the order given, then the exchange sum"""
    acc = np.zeros(64)
    for v, i in zip(vals, idx):
        acc[i % 64] += v
    return _pairwise64(acc)


def decay_chunked(flat, row, nb, mutant=None):
    """One row of rir_decay_kernel on the flat bins buffer (NaN past its end) -> the 7 parameters"""
    def at(i):
        return flat[row * nb + i] if row * nb + i < flat.size else np.nan
    E = flat[row * nb:(row + 1) * nb]
    chunks = -(-nb // DECAY_CHUNK)
    total = _lane_sum(E, np.arange(nb))
    edc = np.zeros(nb)
    carry = 0.0
    for c in range(chunks - 1, -1, -1):
        i = c * 64 + np.arange(64)
        v = np.array([(at(k) if (k < nb or mutant == DECAY_MUTANTS[1]) else 0.0) for k in i])
        s = v.copy()
        o = 1
        while o < 64:                                                        # the shuffle-down scan: s[lane] = sum of v[lane ..]
            t = np.concatenate([s[o:], np.zeros(o)])
            s = s + t
            o <<= 1
        ok = i < nb
        edc[i[ok]] = (s + carry)[ok]
        carry = 0.0 if mutant == DECAY_MUTANTS[0] else carry + s[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = edc / total
        lv = 10.0 * np.log10(np.where(ratio > 1.0, 1.0, ratio))
        out = np.full(7, np.nan)
        order = np.concatenate([np.arange(c * 64, min(c * 64 + 64, nb)) for c in range(chunks - 1, -1, -1)])      # the order a lane meets its bins in
        for r, (lo, hi) in enumerate(R.RANGES):
            sel = order[(lv[order] <= lo) & (lv[order] >= hi)]
            if sel.size:
                pivot = 0.5 * (float(sel.min()) + float(sel.max()))
                x = sel.astype(np.float64) - pivot
                n, sx, sy, sxx, sxy = (_lane_sum(q, sel) for q in (np.ones(sel.size), x, lv[sel], x * x, x * lv[sel]))
                slope = (n * sxy - sx * sy) / (n * sxx - sx * sx) * 1000.0
                out[r] = -60.0 / slope if n >= 2.0 else np.nan
        e50, l50 = _lane_sum(E[order[order < 50]], order[order < 50]), _lane_sum(E[order[order >= 50]], order[order >= 50])
        e80, l80 = _lane_sum(E[order[order < 80]], order[order < 80]), _lane_sum(E[order[order >= 80]], order[order >= 80])
        ts = _lane_sum((order.astype(np.float64) + 0.5) / 1000.0 * E[order], order)
        out[3], out[4], out[5], out[6] = 10.0 * np.log10(e50 / l50), 10.0 * np.log10(e80 / l80), e50 / total, ts / total
    return out


def decay_restated(E, mutant=None):
    """[rows, nb] -> [rows, 7]"""
    flat = np.ascontiguousarray(E, dtype=np.float64).reshape(-1)
    return np.stack([decay_chunked(flat, r, E.shape[1], mutant) for r in range(E.shape[0])])


DECAY_MUTANT_ROWS = {DECAY_MUTANTS[0]: tuple(n for n in DECAY_TABLES if DECAY_TABLES[n].shape[1] >= 65),
                     DECAY_MUTANTS[1]: tuple("nb%d.rows%d" % (nb, rows) for nb in (63, 65, 129) for rows in DECAY_ROW_COUNTS)}
