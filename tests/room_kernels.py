"""RoomSimulator's kernel path by path (TEST INFRASTRUCTURE): csrc/room_sim.hip room_sim_kernel -- the table of test rows, the cells the rows
must reach, the kernel's own image enumeration restated (kernel_images), the float32 restatement fed from those lists in list order
(simulate_f32_listed), the brute-force cube the enumeration is held against (brute_images), and named mutants of the enumeration and of the
arithmetic.  tests/room_ref.py keeps the definition (simulate_f64), the scale s and TAU.

tests/test_gpu_room_kernels.py runs every row through m2h_room_sim against simulate_f64; tests/test_room_kernels_cpu.py checks without a GPU
that the rows reach every cell, that on a seeded sweep of tiles the restated enumeration holds no duplicate, no image above the order and
every image of the brute-force cube that has a tap in the tile, that the listed restatement stays under its kind's ceiling on every row,
that every mutant leaves the bound on the rows named for it by MIN_MARGIN at the least, and that the restated constants are the source's.

Rules (tests/render_kernels.py states them): every element is compared, |g - r| <= tau s with s = the sum over the images of |A w| at that
sample, an element with s = 0 must be exactly 0; the parameters lie inside a NaN-filled buffer and the output is NaN before the call.

A row is one RIR: (room, beta, source, listener, yaw, taps, max_order), room_ref's tuple.

The restated enumeration.  kernel_images(rir, t0) follows the source statement by statement in float64: r_hi, r_lo, mcap, mxlo .. myhi, the
pair order pid % NX, pid / NX, rem_hi, rem_lo, the 1e-12 split, ceil and floor of (+-z - a) inv, the caps olo / ohi with C's division (towards
zero), the run order r = 0 .. 3, the wave scan, and the list slot of every image; pairs are taken ROOM_THREADS at a time (a batch), a batch's
list ROOM_CHUNK slots at a time.  The kernel adds the taps of a sample over the 64 images of a list group (slots 64 g .. 64 g + 63 of a
batch) in slot order, and the group sums in list order: simulate_f32_listed does the same in float32.  (The enumeration is not compiled under
fp contract(off): a fused rem_hi may move an image at the very edge of the shell -- 1 mm outside every tap -- into or out of the list.  That
changes no tap.)

Kinds and taus.  "room": room_ref.TAU = 8 x room_ref.RESTATEMENT_WORST, unchanged.  "dense" (the 0.5 m cube, thousands of taps per sample
summed in float32): a ceiling of its own, DENSE_WORST, pinned by the CPU test, tau = 8 x that.  Never the GPU's own number.

Rows beyond the issue's, and departures, each with its reason:
  + at_left_ear: the source exactly at the left ear (yaw 0, source = listener + (0, HEAD_RADIUS, 0), the same float64 sum the kernel forms):
    d = 0, tau = 0 and the tap at sample 0 has x == 0 exactly.  None of the issue's rows lands a tap on an integer delay, and the cell list
    asks for one; the row also takes the d > 0 ? .. : 1 arm of the ear pattern.
  mutant "second run of a split pair taken from zlo = 0": read literally (b_lo = ceil((0 - a) inv)) the second run gains the images inside the
    hole |Z| < zlo.  They lie nearer than the tile's shell, the integer tap test gives them no tap, and the output does not change: an allowed
    superset, which no bound can reject.  The mutant here is the one that duplicates: the first run is not cut at -zlo (it runs to +zhi, as
    for an unsplit pair) and the second run is kept, so the images of [zlo, zhi] stand in the list twice.
  mutant "ROOM_SHELL_MARGIN and the head radius dropped": the issue names every every-order row.  What the thinner shell loses are images
    whose head centre lies up to HEAD_RADIUS (4.08 samples) outside it while one ear is inside: their taps in the tile have |x| >= 37, where
    the window leaves 2e-4 of A.  Against s that is MIN_MARGIN tau only where few images overlap or several coincide: corner_source (the
    source in a corner, eight images in one place: 164 tau) and at_left_ear (6.2 tau).  On the other every-order rows the bound cannot see
    it (listener_is_source 0.03, yaw+7 0.32, yaw-7 0.83, beta_ones 2.3, beta_zeros_and_one 0.03, slab 0.22, dense 0.04 tau): they are
    not named.  The sweep of the CPU test is what holds the shell: every image of the cube with a tap in the tile must be listed.
  mutant "pz1 lower cap -(left / 2)": C's division makes -((left - 1) / 2) and -(left / 2) equal for odd left; they differ for even
    left >= 2, and the mutant drops the left = 0 arm too (olo = 0 where the source has 1: the empty range), which every order shows.  Named
    for the odd orders but order7: its 700 taps (15 m) end before an image of order 8, all the mutant adds, arrives louder than 0.03 tau s.
  dense: the issue measured 3.1e-6 for simulate_f32, which adds the images of a sample in the cube's order.  In the kernel's list order (64
    images, then the group sums) the float32 sum is a blocked one and the restatement stands at 5.5e-7: the dense kind keeps a ceiling of
    its own, pinned by the CPU test, and it is LOWER than the room kind's (tau 4.8e-6 against 1.36e-5).

Measured on the CPU (python -m pytest tests/test_room_kernels_cpu.py -s): see the header of that file.
"""
import math

import numpy as np

import room_ref as R

F32 = np.float32

# ---- the restated constants of csrc/room_sim.hip (tests/test_room_kernels_cpu.py parses them from the source)
ROOM_TILE, ROOM_THREADS, ROOM_CHUNK, ROOM_HALF_WIDTH = 512, 512, 1024, 41
ROOM_SHELL_MARGIN, ROOM_MIN_SIDE, ROOM_FAR = 1.0e-3, 0.5, 1 << 29
ROOM_RATE, ROOM_C, ROOM_HEAD_RADIUS, ROOM_EAR_PATTERN = 16000.0, 343.0, 0.0875, 0.3
SPLIT_EPS = 1.0e-12
PAD = 1000

MIN_MARGIN = 4.0
DENSE_WORST = 6.0e-7             # the ceiling of simulate_f32_listed's worst |g - r| / s on the dense rows; measured 5.51e-7 (dense); the CPU test pins it
RESTATEMENT_WORST = {"room": R.RESTATEMENT_WORST, "dense": DENSE_WORST}
TAU = {"room": R.TAU, "dense": 8 * DENSE_WORST}

ENUM_MUTANTS = ("pz1 lower cap -(left / 2)", "pz1 upper cap left / 2", "mcap = max_order / 2", "second run of a split pair duplicates",
                "shell margin and head radius dropped", "images past a thread's first chunk dropped", "oxy test dropped",
                "scan exclusive of the lower waves' totals")
MUTANTS = ENUM_MUTANTS + R.MUTANTS


def tau_of(kind):
    return TAU[kind]


# ----------------------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------------------
_ROOM, _BETA = (5.0, 4.0, 3.0), (0.9, 0.7, 0.8, 0.85, 0.5, 0.6)
_SRC, _LIS, _YAW = (4.0, 3.0, 1.0), (1.0, 1.0, 1.2), 0.5
_SLAB_D = (253952 - 35) * 343.0 / 16000.0
_DENSE = dict(room=(0.5, 0.5, 0.5), beta=(0.95, 0.9, 0.92, 0.97, 0.9, 0.99), src=(0.1, 0.2, 0.3), lis=(0.4, 0.3, 0.2), yaw=1.0)
DENSE_TAPS = 600                 # (the issue allows 200 .. 600; the GPU test's header says what was measured)


def _row(name, taps, order, room=_ROOM, beta=_BETA, src=_SRC, lis=_LIS, yaw=_YAW, kind="room"):
    rir = tuple(np.asarray(v, dtype=np.float64) for v in (room, beta, src, lis)) + (float(yaw), int(taps), order)
    return dict(id=name, kind=kind, rir=rir)


ROWS = ([_row("order%d" % n, 1400, n) for n in (1, 2, 3, 4, 5)] + [_row("order7", 700, 7)] +
        [_row("slab", 256000, None, room=(6000.0, 2800.0, 0.5), beta=(0.9, 0.8, 0.7, 0.6, 1.0, 0.999), src=(100.0, 300.0, 0.2),
              lis=(100.0 + math.sqrt(_SLAB_D * _SLAB_D - 0.01), 300.0, 0.3), yaw=0.3),
         _row("wall_x0.order3", 1400, 3, src=(0.0, 3.0, 1.0)),
         _row("corner_source", 1400, None, src=(5.0, 4.0, 3.0)),
         _row("listener_is_source", 700, None, src=(2.0, 1.5, 1.3), lis=(2.0, 1.5, 1.3)),
         _row("corner_listener.order4", 1400, 4, lis=(0.0, 0.0, 0.0)),
         _row("yaw+7", 700, None, yaw=7.0), _row("yaw-7", 700, None, yaw=-7.0),
         _row("beta_ones", 1025, None, beta=(1.0,) * 6),
         _row("beta_zeros_and_one", 1025, None, beta=(0.0, 0.9, 0.8, 0.0, 0.7, 1.0)),
         _row("at_left_ear", 700, None, src=(2.0, 1.5 + 0.0875 * 1.0, 1.3), lis=(2.0, 1.5, 1.3), yaw=0.0),
         _row("dense", DENSE_TAPS, None, kind="dense", **_DENSE), _row("dense.order5", DENSE_TAPS, 5, kind="dense", **_DENSE)])
ROWS_BY_ID = {r["id"]: r for r in ROWS}
BATCH_ROWS = ("slab", "order1", "order3", "dense.order5")        # run solo, then at the last place of a batch of 3 whose other rows differ


def batch_fillers(row):
    """two RIRs with the row's taps and max_order and other parameters"""
    room, beta, src, lis, yaw, taps, order = row["rir"]
    if row["id"] == "slab":
        a = (np.array([3000.0, 2500.0, 1800.0]), np.array([0.9, 0.8, 0.85, 0.95, 0.7, 0.9]), np.array([300.0, 900.0, 400.0]), np.array([850.0, 1100.0, 500.0]), 0.7)
        b = (room, beta, np.array([2100.0, 1300.0, 0.4]), np.array([700.0, 2000.0, 0.1]), -2.0)
    else:
        a = tuple(np.asarray(v, dtype=np.float64) for v in (_ROOM, _BETA, (2.0, 1.5, 1.3), (2.0, 1.5, 1.3))) + (7.0,)
        b = tuple(np.asarray(v, dtype=np.float64) for v in ((7.3, 3.1, 2.6), (0.5, 0.6, 0.7, 0.8, 0.9, 1.0), (6.0, 1.0, 1.0), (2.0, 1.7, 1.3))) + (1.1,)
    return [a + (taps, order), b + (taps, order)]


def pack(rirs):
    """[Q, 16] float64: the parameter rows m2h_room_sim reads"""
    return np.stack([np.concatenate([room, beta, src, lis, [yaw]]) for room, beta, src, lis, yaw, _, _ in rirs])


_REF = {}


def reference(row):
    """(h, s) [taps, 2] float64 of the definition, computed once and left unchanged"""
    if row["id"] not in _REF:
        h, s = R.simulate_f64(row["rir"])
        h.setflags(write=False), s.setflags(write=False)
        _REF[row["id"]] = (h, s)
    return _REF[row["id"]]


def compare(g, r, s, tau):
    """-> (worst |g - r| / s, holds, elements compared): every element; s = 0 asks for an exact 0, a NaN never holds"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    r, s = np.asarray(r).reshape(-1), np.asarray(s).reshape(-1)
    assert g.size == r.size == s.size, (g.size, r.size, s.size)
    if not np.isfinite(g).all():
        return float("inf"), False, g.size
    worst = R.ratio(g, r, s)
    return worst, worst <= tau, g.size


# ----------------------------------------------------------------------------------------------------------------------------------
# the kernel's enumeration, restated
# ----------------------------------------------------------------------------------------------------------------------------------
def _cdiv2(v):
    """v / 2 as C divides ints: towards zero"""
    v = np.asarray(v)
    return np.where(v >= 0, v // 2, -((-v) // 2))


def ntiles_of(taps):
    return (taps + ROOM_TILE - 1) // ROOM_TILE


def kernel_images(rir, t0, mutant=None, cells=None):
    """The list of tile t0 in list order -> dict(dx, dy, dz: 2 m + p per axis; batch: the pair batch; slot: the list slot inside the batch;
    thread) of int64 arrays, plus npairs.  `cells`: a set that takes the names of the branches this tile reaches."""
    room, beta, src, lis, yaw, taps, order = rir
    max_order = -1 if order is None else int(order)
    Lx, Ly, Lz = (float(v) for v in room)
    sx, sy, sz = (float(v) for v in src)
    lx, ly, lz = (float(v) for v in lis)
    tend = min(t0 + ROOM_TILE, taps)
    cr = ROOM_C / ROOM_RATE
    if mutant == ENUM_MUTANTS[4]:
        r_hi = float(tend + ROOM_HALF_WIDTH - 1) * cr
        r_lo = max(float(t0 - ROOM_HALF_WIDTH) * cr, 0.0)
    else:
        r_hi = float(tend + ROOM_HALF_WIDTH - 1) * cr + ROOM_HEAD_RADIUS + ROOM_SHELL_MARGIN
        r_lo = max(float(t0 - ROOM_HALF_WIDTH) * cr - ROOM_HEAD_RADIUS - ROOM_SHELL_MARGIN, 0.0)
    mcap = (max_order // 2 + (0 if mutant == ENUM_MUTANTS[2] else 1)) if max_order >= 0 else ROOM_FAR
    mxlo, mxhi = max(int(math.floor((lx - r_hi - abs(sx)) / (2.0 * Lx))), -mcap), min(int(math.ceil((lx + r_hi + abs(sx)) / (2.0 * Lx))), mcap)
    mylo, myhi = max(int(math.floor((ly - r_hi - abs(sy)) / (2.0 * Ly))), -mcap), min(int(math.ceil((ly + r_hi + abs(sy)) / (2.0 * Ly))), mcap)
    NX, NY = max(2 * (mxhi - mxlo + 1), 0), max(2 * (myhi - mylo + 1), 0)
    npairs = NX * NY
    out = {k: [] for k in ("dx", "dy", "dz", "batch", "slot", "thread")}
    if cells is not None:
        cells.add("partial last tile" if tend - t0 < ROOM_TILE else "whole tile")
        if npairs > ROOM_THREADS:
            cells.add("npairs > 512: more than one pair batch")
    nlisted = 0
    for bi, pb in enumerate(range(0, npairs, ROOM_THREADS)):
        pid = np.arange(pb, min(pb + ROOM_THREADS, npairs), dtype=np.int64)
        nt = pid.size
        ix, iy = pid % NX, pid // NX
        px, mx, py, my = ix & 1, mxlo + (ix >> 1), iy & 1, mylo + (iy >> 1)
        dxc, dyc = mx * 2 + px, my * 2 + py
        X = (1 - 2 * px).astype(np.float64) * sx + (2 * mx).astype(np.float64) * Lx - lx
        Y = (1 - 2 * py).astype(np.float64) * sy + (2 * my).astype(np.float64) * Ly - ly
        oxy = np.abs(mx - px) + np.abs(mx) + np.abs(my - py) + np.abs(my)
        rem_hi, rem_lo = r_hi * r_hi - X * X - Y * Y, r_lo * r_lo - X * X - Y * Y
        under = (max_order < 0) | (oxy <= max_order)
        live = (rem_hi >= 0.0) & (under | (mutant == ENUM_MUTANTS[6]))
        zhi = np.sqrt(np.maximum(rem_hi, 0.0))
        split = rem_lo > SPLIT_EPS
        zlo = np.where(split, np.sqrt(np.maximum(rem_lo, 0.0)), 0.0)
        left = max_order - oxy
        cnt, first = np.zeros((nt, 4), dtype=np.int64), np.zeros((nt, 4), dtype=np.int64)
        inv = 1.0 / (2.0 * Lz)
        for pz in range(2):
            a = float(1 - 2 * pz) * sz - lz
            olo, ohi = np.full(nt, -ROOM_FAR, dtype=np.int64), np.full(nt, ROOM_FAR, dtype=np.int64)
            if max_order >= 0:
                if pz == 0:
                    olo, ohi = -_cdiv2(left), _cdiv2(left)
                else:
                    olo = -_cdiv2(left) if mutant == ENUM_MUTANTS[0] else np.where(left >= 1, -_cdiv2(left - 1), 1)
                    ohi = _cdiv2(left) if mutant == ENUM_MUTANTS[1] else _cdiv2(left + 1)
            first_end = zhi if mutant == ENUM_MUTANTS[3] else np.where(split, -zlo, zhi)
            g_lo, g_hi = np.ceil((-zhi - a) * inv).astype(np.int64), np.floor((first_end - a) * inv).astype(np.int64)
            a_lo, a_hi = np.maximum(g_lo, olo), np.minimum(g_hi, ohi)
            first[:, 2 * pz], cnt[:, 2 * pz] = a_lo, np.maximum(a_hi - a_lo + 1, 0)
            h_lo, h_hi = np.ceil((zlo - a) * inv).astype(np.int64), np.floor((zhi - a) * inv).astype(np.int64)
            b_lo, b_hi = np.maximum(h_lo, olo), np.minimum(h_hi, ohi)
            first[:, 2 * pz + 1], cnt[:, 2 * pz + 1] = b_lo, np.where(split, np.maximum(b_hi - b_lo + 1, 0), 0)
            if cells is not None and max_order >= 0 and live.any():
                lv = left[live]
                if pz == 0:
                    arms = (("pz0 cap, left even", lv % 2 == 0), ("pz0 cap, left odd", lv % 2 == 1))
                else:
                    arms = (("pz1 cap, left = 0: the empty range", lv == 0), ("pz1 cap, left odd", lv % 2 == 1), ("pz1 cap, left even >= 2", (lv % 2 == 0) & (lv >= 2)))
                cells.update(name for name, hit in arms if hit.any())
                cut = live & (((g_lo < olo) & (g_hi >= olo)) | ((g_hi > ohi) & (g_lo <= ohi)) | (split & (((h_lo < olo) & (h_hi >= olo)) | ((h_hi > ohi) & (h_lo <= ohi)))))
                if cut.any():
                    cells.add("pz%d cap cuts a run that geometry leaves longer" % pz)
        cnt[~live] = 0
        if cells is not None:
            if max_order >= 0:
                if (live & split).any():
                    cells.add("split under a cap")
                if (live & ~split).any():
                    cells.add("no split under a cap")
                if ((rem_hi >= 0.0) & ~under).any():
                    cells.add("pair inside the disc refused by oxy > max_order")
            else:
                cells.add("no cap: every order")
                if (live & split).any():
                    cells.add("split, every order")
        mine = cnt.sum(1)
        incl = np.cumsum(mine)
        off, total = incl - mine, int(incl[-1])
        if total == 0:
            continue
        flat = cnt.reshape(-1)
        run = np.repeat(np.arange(nt * 4), flat)
        within = np.arange(total) - np.repeat(np.cumsum(flat) - flat, flat)
        thread = run // 4
        dz = (first.reshape(-1)[run] + within) * 2 + ((run % 4) >> 1)
        slot = np.arange(total, dtype=np.int64)
        keep = np.ones(total, dtype=bool)
        if cells is not None:
            if (mine > ROOM_CHUNK).any():
                cells.add("mine > ROOM_CHUNK: a thread's images over more than one chunk")
            if total > ROOM_CHUNK:
                b = np.arange(ROOM_CHUNK, total, ROOM_CHUNK)
                if (run[b] == run[b - 1]).any():
                    cells.add("total > ROOM_CHUNK, a chunk border inside a run")
        if mutant == ENUM_MUTANTS[5]:
            keep = slot // ROOM_CHUNK == off[thread] // ROOM_CHUNK
        if mutant == ENUM_MUTANTS[7]:                                       # the slots of wave w start at 0 again: the highest thread's image stays in a slot
            wave0 = off[(np.arange(nt) // 64) * 64]
            slot = slot - wave0[thread]
            _, last = np.unique(slot[::-1], return_index=True)
            keep = np.zeros(total, dtype=bool)
            keep[total - 1 - last] = True
        order_ix = np.argsort(slot[keep], kind="stable")
        for k, v in (("dx", dxc[thread]), ("dy", dyc[thread]), ("dz", dz), ("batch", np.full(total, bi, dtype=np.int64)), ("slot", slot), ("thread", thread)):
            out[k].append(v[keep][order_ix])
        nlisted += int(keep.sum())
    if cells is not None and nlisted == 0:
        cells.add("empty tile")
    res = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64)) for k, v in out.items()}
    res["npairs"] = npairs
    return res


def decode(code):
    """2 m + p -> p, m"""
    return code & 1, code >> 1


def exponents(dx, dy, dz):
    """[N, 6] in the wall order of beta"""
    cols = []
    for c in (dx, dy, dz):
        p, m = decode(c)
        cols += [np.abs(m - p), np.abs(m)]
    return np.stack(cols, 1) if len(dx) else np.zeros((0, 6), dtype=np.int64)


def positions(rir, dx, dy, dz):
    room, _, src = rir[:3]
    cols = []
    for a, c in enumerate((dx, dy, dz)):
        p, m = decode(c)
        cols.append((1 - 2 * p).astype(np.float64) * float(src[a]) + (2 * m).astype(np.float64) * float(room[a]))
    return np.stack(cols, 1) if len(dx) else np.zeros((0, 3))


def key_of(dx, dy, dz):
    """one int64 per image"""
    B = 1 << 20
    return ((dx + B // 2) * B + (dy + B // 2)) * B + (dz + B // 2)


def brute_images(rir):
    """Every image of the cube about the reach sphere of [0, taps), by the definition alone -> dx, dy, dz, order, k [N, 2] (the delay floor per ear)"""
    room, beta, src, lis, yaw, taps, order = rir
    rmax = R.C * (taps + R.HALF_WIDTH) / R.RATE + R.HEAD_RADIUS + 1e-6
    ax = []
    for a in range(3):
        M = int(math.ceil((rmax + room[a]) / (2.0 * room[a]))) + 1
        m, p = np.repeat(np.arange(-M, M + 1), 2), np.tile(np.array([0, 1]), 2 * M + 1)
        x = (1 - 2 * p) * src[a] + 2 * m * room[a]
        keep = np.abs(x - lis[a]) <= rmax
        ax.append((x[keep], (2 * m + p)[keep], (np.abs(m - p) + np.abs(m))[keep]))
    ix, iy = (v.ravel() for v in np.meshgrid(np.arange(len(ax[0][0])), np.arange(len(ax[1][0])), indexing="ij"))
    if order is not None:
        keep = ax[0][2][ix] + ax[1][2][iy] <= order
        ix, iy = ix[keep], iy[keep]
    r2 = rmax * rmax - (ax[0][0][ix] - lis[0]) ** 2 - (ax[1][0][iy] - lis[1]) ** 2
    ix, iy, r2 = ix[r2 >= 0], iy[r2 >= 0], r2[r2 >= 0]
    nz = len(ax[2][0])
    ix, iy, r2 = np.repeat(ix, nz), np.repeat(iy, nz), np.repeat(r2, nz)
    iz = np.tile(np.arange(nz), len(ix) // max(nz, 1))
    keep = (ax[2][0][iz] - lis[2]) ** 2 <= r2
    ix, iy, iz = ix[keep], iy[keep], iz[keep]
    n = ax[0][2][ix] + ax[1][2][iy] + ax[2][2][iz]
    if order is not None:
        keep = n <= order
        ix, iy, iz, n = ix[keep], iy[keep], iz[keep], n[keep]
    pos = np.stack([ax[0][0][ix], ax[1][0][iy], ax[2][0][iz]], 1)
    k = np.zeros((len(ix), 2), dtype=np.int64)
    for e, (ear, _) in enumerate(R._ears(lis, yaw)):
        v = pos - ear[None, :]
        k[:, e] = np.floor(np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]) * R.RATE / R.C).astype(np.int64)
    return ax[0][1][ix], ax[1][1][iy], ax[2][1][iz], n, k


# ----------------------------------------------------------------------------------------------------------------------------------
# the float32 restatement, fed from the kernel's lists
# ----------------------------------------------------------------------------------------------------------------------------------
def _tile_f32(rir, t0, img, mutant, cells):
    """-> [tend - t0, 2] float32: steps 2 and 3 of the kernel on one tile's list"""
    room, beta, src, lis, yaw, taps, order = rir
    tend = min(t0 + ROOM_TILE, taps)
    T = tend - t0
    dx, dy, dz = img["dx"], img["dy"], img["dz"]
    exps = exponents(dx, dy, dz)
    if mutant == "walls_swapped":
        exps = exps[:, [1, 0, 3, 2, 5, 4]]
    if mutant == "order_lt" and order is not None:
        sel = exps.sum(1) < order
        img = {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in img.items()}
        dx, dy, dz, exps = img["dx"], img["dy"], img["dz"], exps[sel]
    N = len(dx)
    if N == 0:
        return np.zeros((T, 2), dtype=F32)
    pos = positions(rir, dx, dy, dz)
    with np.errstate(divide="ignore"):
        lg = np.maximum(np.log2(beta), -1.0e6)
    arg = np.zeros(N)
    for w in range(6):
        arg = arg + exps[:, w].astype(np.float64) * lg[w]
    ai = np.floor(arg)
    G = np.ldexp(np.exp2((arg - ai).astype(F32)), np.minimum(np.maximum(ai, -400.0), 400.0).astype(np.int64)).astype(F32)
    if cells is not None:
        for w in range(6):
            if beta[w] == 0 and (exps[:, w] == 0).any():
                cells.add("beta = 0 with exponent 0")
            if beta[w] == 0 and (exps[:, w] > 0).any():
                cells.add("beta = 0 with exponent > 0")
    hw = 40 if mutant == "half_width_40" else ROOM_HALF_WIDTH
    jt = np.arange(-hw - 1, hw + 2)
    tab_c, tab_s = np.cos(math.pi * jt / (2.0 * hw)).astype(F32), np.sin(math.pi * jt / (2.0 * hw)).astype(F32)
    # list groups: 64 slots of a batch; the batches in order
    grp_in_batch = img["slot"] // 64
    nb = int(img["batch"].max()) + 1
    per_batch = np.zeros(nb + 1, dtype=np.int64)
    np.maximum.at(per_batch, img["batch"] + 1, grp_in_batch + 1)
    grp = np.cumsum(per_batch)[img["batch"]] + grp_in_batch
    lane = img["slot"] % 64
    acc = np.zeros((int(grp.max()) + 1, T, 2), dtype=F32)
    vals, ns, oks = [], [], []
    for e, (ear, axis) in enumerate(R._ears(lis, yaw)):
        v = pos - ear[None, :]
        d = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        cos = np.where(d > 0, (v[:, 0] * axis[0] + v[:, 1] * axis[1]) / np.where(d > 0, d, 1.0), 1.0)
        with np.errstate(divide="ignore"):
            A = (((1.0 - ROOM_EAR_PATTERN) + ROOM_EAR_PATTERN * cos) / (4.0 * math.pi * (d if mutant == "no_clamp" else np.maximum(d, ROOM_HEAD_RADIUS)))).astype(F32) * G
        if mutant == "split_f32":
            tau = d.astype(F32) * F32(ROOM_RATE) / F32(ROOM_C)
            k, kr = np.floor(tau), np.floor(tau + F32(0.5))
        else:
            tau = d * ROOM_RATE / ROOM_C
            k, kr = np.floor(tau), np.floor(tau + 0.5)
        fr = (tau - kr).astype(F32)
        k, kr = k.astype(np.int64), kr.astype(np.int64)
        sp = -(A * np.sin(F32(math.pi) * fr)) / F32(math.pi)
        cf, sf = np.cos(F32(math.pi / (2.0 * hw)) * fr), np.sin(F32(math.pi / (2.0 * hw)) * fr)
        firstn = -41 if mutant == "taps_shifted" else -40
        n = k[:, None] + np.arange(firstn, firstn + 82)[None, :]
        ok = (n >= t0) & (n < tend)                                        # the tap test, exact in integers
        j = n - kr[:, None]
        x = j.astype(F32) - fr[:, None]
        jj = np.clip(j + hw + 1, 0, len(jt) - 1)
        c = tab_c[jj] * cf[:, None] + tab_s[jj] * sf[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(x == 0, A[:, None], np.where(j % 2 == 0, sp[:, None], -sp[:, None]) / x)
        val = (q * c * c).astype(F32)
        if cells is not None:
            if (d < ROOM_HEAD_RADIUS).any():
                cells.add("d < HEAD_RADIUS")
            if (ok & (x == 0)).any():
                cells.add("x == 0 exactly: a tap on an integer delay")
        vals.append(val), ns.append(n - t0), oks.append(ok)
    ear_out = [1, 0] if mutant == "ears_swapped" else [0, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(64):
            sel = np.nonzero(lane == p)[0]
            if sel.size == 0:
                continue
            for e in range(2):
                okk = oks[e][sel]
                gg = np.broadcast_to(grp[sel][:, None], okk.shape)[okk]
                acc[gg, ns[e][sel][okk], ear_out[e]] += vals[e][sel][okk]      # one image per (group, lane): no index twice
        h = np.zeros((T, 2), dtype=F32)
        for g in range(acc.shape[0]):
            h += acc[g]
    return h


def simulate_f32_listed(rir, mutant=None, cells=None):
    """The arithmetic of room_ref.simulate_f32 fed tile by tile from kernel_images, the images added in list order as the kernel adds them.
    `mutant`: one of MUTANTS.  `cells`: a set that takes every cell the row reaches.  -> h [taps, 2] float32"""
    taps = rir[5]
    h = np.zeros((taps, 2), dtype=F32)
    enum_mutant = mutant if mutant in ENUM_MUTANTS else None
    for t0 in range(0, taps, ROOM_TILE):
        img = kernel_images(rir, t0, enum_mutant, cells)
        h[t0:t0 + ROOM_TILE] = _tile_f32(rir, t0, img, mutant, cells)
    return h


ALL_CELLS = frozenset((
    "no cap: every order", "split, every order", "pz0 cap, left even", "pz0 cap, left odd", "pz1 cap, left = 0: the empty range", "pz1 cap, left odd",
    "pz1 cap, left even >= 2", "pz0 cap cuts a run that geometry leaves longer", "pz1 cap cuts a run that geometry leaves longer", "split under a cap",
    "no split under a cap", "pair inside the disc refused by oxy > max_order", "mine > ROOM_CHUNK: a thread's images over more than one chunk",
    "npairs > 512: more than one pair batch", "total > ROOM_CHUNK, a chunk border inside a run", "empty tile", "partial last tile", "whole tile",
    "d < HEAD_RADIUS", "x == 0 exactly: a tap on an integer delay", "beta = 0 with exponent 0", "beta = 0 with exponent > 0"))

_odd = ("order1", "order3", "order5", "order7", "wall_x0.order3")
_odd_full = ("order1", "order3", "order5", "wall_x0.order3")     # (order7 runs 700 taps, 15 m: no image of order 8, the mutant's gain, arrives louder than 0.03 tau s)
# mutant -> the rows the bound must reject it on
MUTANT_ROWS = {
    ENUM_MUTANTS[0]: _odd_full, ENUM_MUTANTS[1]: _odd, ENUM_MUTANTS[2]: ("order1",), ENUM_MUTANTS[3]: ("order3", "corner_source", "order5"),
    ENUM_MUTANTS[4]: ("corner_source", "at_left_ear"),
    ENUM_MUTANTS[5]: ("slab",), ENUM_MUTANTS[6]: ("order2",), ENUM_MUTANTS[7]: ("order5", "corner_source", "dense.order5"),
    "split_f32": ("slab",), "walls_swapped": ("order3",), "ears_swapped": ("yaw+7", "order1"), "half_width_40": ("order1",), "taps_shifted": ("order1",),
    "order_lt": ("order2", "order5"), "no_clamp": ("at_left_ear",),
}
