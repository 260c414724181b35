"""RoomSimulator's definition in float64 numpy (m2h/audio/room.py states it), the float32 restatement of the arithmetic of
csrc/room_sim.hip, the named cases of the CPU and the GPU tests, the mutants and the element bound.

Definition.  An image of the source s in the room (Lx, Ly, Lz) is indexed by p in {0, 1}^3 and m in Z^3: along an axis its coordinate is
(1 - 2 p) s + 2 m L, it has |m - p| reflections on the wall at 0 and |m| on the wall at L, its gain is the product over the axes of
beta_lo^|m - p| beta_hi^|m| (0^0 = 1) and its order the sum of the six exponents; max_order = N keeps the orders <= N.  With
u = (-sin yaw, cos yaw, 0) the left ear (e = 0) is at listener + HEAD_RADIUS u with axis +u, the right at listener - HEAD_RADIUS u with
axis -u; v = image - ear, d = |v|, cos = v . axis / d (1 at d = 0), A = G (0.7 + 0.3 cos) / (4 pi max(d, HEAD_RADIUS)).  tau = d RATE / C,
k = floor(tau); the image adds A sinc(x) (1 + cos(pi x / 41)) / 2, x = n - tau, to h[n, e] for n = k - 40 .. k + 41 inside [0, taps).

Bound.  |g - r| <= TAU s per element, s = the sum over the images of |A w| at that sample (simulate_f64 returns it), TAU = 8 x the worst
ratio of the float32 restatement over the cases (RESTATEMENT_WORST, measured on the CPU and pinned in tests/test_room_cpu.py)."""
import math

import numpy as np

RATE = 16000
C = 343.0
HEAD_RADIUS = 0.0875
HALF_WIDTH = 41
EAR_PATTERN = 0.3
MAX_TAPS = 256000
TILE = 512                       # ops.ROOM_TILE: output samples of a workgroup of csrc/room_sim.hip

RESTATEMENT_WORST = 1.7e-6       # the ceiling of simulate_f32's worst |g - r| / s over cases(); measured 1.652e-6 (moving); tests/test_room_cpu.py pins it
TAU = 8 * RESTATEMENT_WORST

MUTANTS = ("split_f32", "walls_swapped", "ears_swapped", "half_width_40", "taps_shifted", "order_lt", "no_clamp")


def _axis(L, b_lo, b_hi, s, l, rmax, max_order, mutant):
    """every (p, m) of one axis whose image can lie within rmax of the listener coordinate l -> coordinate, gain, order"""
    m_lo = int(math.floor((l - rmax - abs(s)) / (2.0 * L))) - 1
    m_hi = int(math.ceil((l + rmax + abs(s)) / (2.0 * L))) + 1
    if max_order is not None:
        m_lo, m_hi = max(m_lo, -(max_order // 2 + 1)), min(m_hi, max_order // 2 + 1)
    m = np.repeat(np.arange(m_lo, m_hi + 1), 2)
    p = np.tile(np.array([0, 1]), m_hi - m_lo + 1)
    x = (1 - 2 * p) * s + 2 * m * L
    e_lo, e_hi = np.abs(m - p), np.abs(m)
    if mutant == "walls_swapped":
        e_lo, e_hi = e_hi, e_lo
    keep = np.abs(x - l) <= rmax
    return x[keep], e_lo[keep], e_hi[keep]


def image_table(room, beta, src, lis, taps, max_order=None, mutant=None):
    """-> pos [N, 3] float64, exponents [N, 6] int64 (wall order of beta) of every image within reach of [0, taps), and the number of
    candidates in the cube around the reach sphere."""
    rmax = C * (taps + HALF_WIDTH) / RATE + HEAD_RADIUS + 1e-6
    ax = [_axis(room[a], beta[2 * a], beta[2 * a + 1], src[a], lis[a], rmax, max_order, mutant) for a in range(3)]
    cube = len(ax[0][0]) * len(ax[1][0]) * len(ax[2][0])
    ix, iy = np.meshgrid(np.arange(len(ax[0][0])), np.arange(len(ax[1][0])), indexing="ij")
    ix, iy = ix.ravel(), iy.ravel()
    r2 = rmax * rmax - (ax[0][0][ix] - lis[0]) ** 2 - (ax[1][0][iy] - lis[1]) ** 2
    keep = r2 >= 0
    ix, iy, r2 = ix[keep], iy[keep], r2[keep]
    nz = len(ax[2][0])
    ix, iy, r2 = np.repeat(ix, nz), np.repeat(iy, nz), np.repeat(r2, nz)
    iz = np.tile(np.arange(nz), len(ix) // max(nz, 1))
    keep = (ax[2][0][iz] - lis[2]) ** 2 <= r2
    ix, iy, iz = ix[keep], iy[keep], iz[keep]
    pos = np.stack([ax[0][0][ix], ax[1][0][iy], ax[2][0][iz]], 1)
    exps = np.stack([ax[0][1][ix], ax[0][2][ix], ax[1][1][iy], ax[1][2][iy], ax[2][1][iz], ax[2][2][iz]], 1)
    if max_order is not None:
        order = exps.sum(1)
        keep = order < max_order if mutant == "order_lt" else order <= max_order
        pos, exps = pos[keep], exps[keep]
    return pos, exps, cube


def _ears(lis, yaw):
    u = np.array([-math.sin(yaw), math.cos(yaw), 0.0])
    return [(lis + HEAD_RADIUS * u, u), (lis - HEAD_RADIUS * u, -u)]


def _taps_of(k, taps, mutant):
    first = -41 if mutant == "taps_shifted" else -40
    n = k[:, None] + np.arange(first, first + 82)[None, :]
    return n, (n >= 0) & (n < taps)


def simulate_f64(rir, mutant=None):
    """rir: one row of rirs_of(case) -> h [taps, 2] float64 and s [taps, 2] = sum of |A w|"""
    room, beta, src, lis, yaw, taps, max_order = rir
    pos, exps, _ = image_table(room, beta, src, lis, taps, max_order, mutant)
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.prod(np.where(exps == 0, 1.0, beta[None, :] ** exps), 1)
    h, s = np.zeros((taps, 2)), np.zeros((taps, 2))
    for e, (ear, axis) in enumerate(_ears(lis, yaw)):
        if mutant == "ears_swapped":
            e = 1 - e
        v = pos - ear[None, :]
        d = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        cos = np.where(d > 0, (v[:, 0] * axis[0] + v[:, 1] * axis[1]) / np.where(d > 0, d, 1.0), 1.0)
        A = G * ((1.0 - EAR_PATTERN) + EAR_PATTERN * cos) / (4.0 * math.pi * (d if mutant == "no_clamp" else np.maximum(d, HEAD_RADIUS)))
        tau = d * RATE / C
        k = np.floor(tau).astype(np.int64)
        n, ok = _taps_of(k, taps, mutant)
        x = n - tau[:, None]
        hw = 40.0 if mutant == "half_width_40" else float(HALF_WIDTH)
        sinc = np.where((x != 0) & (x == np.rint(x)), 0.0, np.sinc(x))      # (a delay that is a whole number: numpy's sin(pi n) / (pi n) is 4e-17, the definition's is 0)
        w = sinc * 0.5 * (1.0 + np.cos(math.pi * x / hw))
        val = A[:, None] * w
        np.add.at(h[:, e], n[ok], val[ok])
        np.add.at(s[:, e], n[ok], np.abs(val[ok]))
    return h, s


_F = np.float32


def simulate_f32(rir, mutant=None):
    """The arithmetic of csrc/room_sim.hip: d, tau, k and the split tau = kr + fr, |fr| <= 1/2, in float64; the gain as
    exp2 of the float64 sum of exponent x log2(beta), split into its integer and its fraction; everything per tap and the sums in float32:
    sin(pi x) = -(-1)^j sin(pi fr), the window cos^2(pi x / 82) by the addition theorem from a float32 table over j.  -> h [taps, 2] float32"""
    room, beta, src, lis, yaw, taps, max_order = rir
    pos, exps, _ = image_table(room, beta, src, lis, taps, max_order, mutant)
    with np.errstate(divide="ignore"):
        lg = np.maximum(np.log2(beta), -1.0e6)
    arg = (exps * lg[None, :]).sum(1)
    ai = np.floor(arg)
    G = np.ldexp(np.exp2((arg - ai).astype(_F)), np.maximum(ai, -400).astype(np.int64)).astype(_F)
    h = np.zeros((taps, 2), dtype=_F)
    hw = 40 if mutant == "half_width_40" else HALF_WIDTH
    jt = np.arange(-hw - 1, hw + 2)
    tab_c, tab_s = np.cos(math.pi * jt / (2.0 * hw)).astype(_F), np.sin(math.pi * jt / (2.0 * hw)).astype(_F)
    for e, (ear, axis) in enumerate(_ears(lis, yaw)):
        if mutant == "ears_swapped":
            e = 1 - e
        v = pos - ear[None, :]
        d = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        cos = np.where(d > 0, (v[:, 0] * axis[0] + v[:, 1] * axis[1]) / np.where(d > 0, d, 1.0), 1.0)
        A = (((1.0 - EAR_PATTERN) + EAR_PATTERN * cos) / (4.0 * math.pi * (d if mutant == "no_clamp" else np.maximum(d, HEAD_RADIUS)))).astype(_F) * G
        if mutant == "split_f32":
            tau = d.astype(_F) * _F(RATE) / _F(C)
            k = np.floor(tau)
            kr = np.floor(tau + _F(0.5))
            fr = (tau - kr).astype(_F)
            k, kr = k.astype(np.int64), kr.astype(np.int64)
        else:
            tau = d * RATE / C
            k = np.floor(tau)
            kr = np.floor(tau + 0.5)
            fr = (tau - kr).astype(_F)
            k, kr = k.astype(np.int64), kr.astype(np.int64)
        sp = -(A * np.sin(_F(math.pi) * fr)) / _F(math.pi)
        cf, sf = np.cos(_F(math.pi / (2.0 * hw)) * fr), np.sin(_F(math.pi / (2.0 * hw)) * fr)
        n, ok = _taps_of(k, taps, mutant)
        j = n - kr[:, None]
        x = j.astype(_F) - fr[:, None]
        jj = np.clip(j + hw + 1, 0, len(jt) - 1)
        c = tab_c[jj] * cf[:, None] + tab_s[jj] * sf[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(x == 0, A[:, None], np.where(j % 2 == 0, sp[:, None], -sp[:, None]) / x)
        val = (q * c * c).astype(_F)
        np.add.at(h[:, e], n[ok], val[ok])
    return h


def ratio(got, ref, s):
    """worst |got - ref| / s; an element with s = 0 must agree exactly (inf otherwise)"""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def beta_from_t60(room, t60):
    V = room[0] * room[1] * room[2]
    S = 2.0 * (room[0] * room[1] + room[1] * room[2] + room[0] * room[2])
    return np.full(6, math.sqrt(math.exp(-0.161 * V / (S * t60))))


def _border_distance(delay):
    """head-centre distance of a source on the left ear's side, in the ear's axis, whose direct delay to the left ear is `delay` samples"""
    return delay * C / RATE + HEAD_RADIUS


def cases():
    """name -> dict(room [R, 3], beta [R, 6], sources [R, S, 3], listener [R, 3] or [R, K, 3], yaw [R] or [R, K], taps, max_order), float64"""
    out = {}
    out["taps1"] = dict(room=[[5.0, 4.0, 3.0]], beta=[[0.9, 0.85, 0.8, 0.9, 0.7, 0.6]], sources=[[[2.3, 2.0, 1.5]]], listener=[[2.0, 2.0, 1.5]], yaw=[0.4],
                        taps=1, max_order=None)
    out["taps700"] = dict(room=[[5.0, 4.0, 3.0], [7.3, 3.1, 2.6], [4.0, 6.0, 2.5]],
                          beta=[[0.9, 0.85, 0.8, 0.9, 0.7, 0.6], [0.0] * 6, [0.5, 0.6, 0.7, 0.8, 0.9, 1.0]],
                          sources=[[[1.0, 2.0, 1.5], [4.1, 0.7, 2.2]], [[6.0, 1.0, 1.0], [0.4, 2.9, 2.0]], [[2.0546, 2.975, 1.2], [3.5, 5.5, 0.3]]],      # (room 2, source 0: 0.0275 m from the left ear)
                          listener=[[3.0, 2.0, 1.5], [2.0, 1.7, 1.3], [2.0, 3.0, 1.2]], yaw=[0.0, 1.1, -2.0], taps=700, max_order=None)
    for half, tag in ((-0.5, "before"), (0.5, "after")):
        D = _border_distance(TILE + half)
        for N in (0, None):
            out["tile_border.%s.%s" % (tag, "order0" if N == 0 else "full")] = dict(
                room=[[5.0, 14.0, 3.0]], beta=[[0.8, 0.7, 0.9, 0.6, 0.75, 0.85]], sources=[[[2.5, 1.5 + D, 1.5]]], listener=[[2.5, 1.5, 1.5]], yaw=[0.0],
                taps=TILE + 82 + 17, max_order=N)
    lis = [[[1.0, 1.0, 1.2], [2.0, 1.5, 1.3], [3.0, 2.0, 1.4]], [[5.0, 2.0, 1.6], [4.0, 2.5, 1.6], [3.0, 3.0, 1.6]]]
    out["moving"] = dict(room=[[5.0, 4.0, 3.0], [8.2, 5.1, 2.7]], beta=[[0.9, 0.7, 0.8, 0.85, 0.5, 0.6], [0.6, 0.95, 0.9, 0.8, 0.7, 0.75]],
                         sources=[[[4.0, 3.0, 1.0], [0.5, 3.5, 2.0]], [[1.0, 1.0, 1.0], [7.0, 4.0, 2.0]]], listener=lis,
                         yaw=[[0.0, 0.5, 1.0], [-1.0, 2.0, 3.0]], taps=3200, max_order=None)
    out["far"] = dict(room=[[3000.0, 2500.0, 1800.0]], beta=[[0.9, 0.8, 0.85, 0.95, 0.7, 0.9]], sources=[[[300.0, 900.0, 400.0]]],
                      listener=[[850.0, 1100.0, 500.0]], yaw=[0.7], taps=256000, max_order=2)
    return {k: {a: (np.asarray(b, dtype=np.float64) if a not in ("taps", "max_order") else b) for a, b in v.items()} for k, v in out.items()}


def rirs_of(case):
    """the RIRs of a case in output order: a list of (room, beta, source, listener, yaw, taps, max_order) and the leading shape"""
    room, beta, src, lis, yaw = (case[k] for k in ("room", "beta", "sources", "listener", "yaw"))
    R_, S = src.shape[:2]
    moving = lis.ndim == 3
    K = lis.shape[1] if moving else 1
    rows = []
    for r in range(R_):
        for s in range(S):
            for k in range(K):
                rows.append((room[r], beta[r], src[r, s], lis[r, k] if moving else lis[r], float(yaw[r, k] if moving else yaw[r]), case["taps"],
                             case["max_order"]))
    return rows, ((R_, S, K) if moving else (R_, S))


_REF = {}


def reference(name):
    """(h [Q, taps, 2], s [Q, taps, 2]) float64 of a named case, computed once"""
    if name not in _REF:
        rows, _ = rirs_of(cases()[name])
        hs = [simulate_f64(r) for r in rows]
        _REF[name] = (np.stack([a for a, _ in hs]), np.stack([b for _, b in hs]))
    return _REF[name]
