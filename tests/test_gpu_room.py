"""GPU: m2h_room_sim (csrc/room_sim.hip) and RoomSimulator against the float64 definition (tests/room_ref.py) inside the element bound
|g - r| <= TAU s that tests/test_room_cpu.py pins, the bits of an RIR against batch, chunking and run, and the output going into the
Auralizer and RoomAcoustics unchanged.

Cases (room_ref.cases()): taps1 (one tap, the source 0.3 m from the head: taps reach sample 0); taps700 (three rooms in one batch, one with
beta = 0, one with the source inside the head radius); tile_border (taps = ROOM_TILE + 82 + 17, the direct delay at ROOM_TILE -+ 0.5, with
max_order = 0 and with every order: taps straddle the tile border, the last tile is partial); moving ([2, 2, 3], taps = 3200, every order,
rooms of different size and unequal walls); far (one RIR of 256000 taps in a 3000 x 2500 x 1800 m room, max_order = 2).  The entry point
reads its parameters from inside a NaN-filled buffer and writes into a NaN-filled one; the wrapper takes views of NaN-filled tensors.
(-s prints every measured ratio.)

Measured on one MI355X, worst |g - r| / s (TAU = 1.36e-5): taps1 1.63e-7, taps700 3.65e-7, tile_border 2.21e-7 .. 2.84e-7, moving 5.65e-7,
far 4.89e-7; the 13 tests before the command-line one in 4.4 s."""
import ctypes

import numpy as np
import pytest
import torch

import acoustics_ref as AR
import room_ref as R
from m2h import _lib, ops
from m2h.audio import room as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = R.cases()
NAMES = ["taps1", "taps700", "tile_border.before.order0", "tile_border.before.full", "tile_border.after.order0", "tile_border.after.full", "moving", "far"]
_CACHE = {}


def _sim():
    if "sim" not in _CACHE:
        _CACHE["sim"] = M.RoomSimulator(DEV)
    return _CACHE["sim"]


def _view(a, dtype=torch.float64):
    """the array as a view of the inside of a NaN-filled tensor one element larger on every side"""
    a = np.asarray(a)
    big = torch.full(tuple(n + 2 for n in a.shape), float("nan"), device=DEV, dtype=dtype)
    inner = big[tuple(slice(1, -1) for _ in a.shape)]
    inner.copy_(torch.from_numpy(a).to(dtype))
    return inner


def _inputs(name, dtype=torch.float64):
    c = CASES[name]
    return [_view(c[k], dtype) for k in ("room", "beta", "sources", "listener", "yaw")]


def _simulate(name, sim=None):
    key = ("out", name)
    if sim is not None:
        return sim.simulate(*_inputs(name), CASES[name]["taps"], max_order=CASES[name]["max_order"])
    if key not in _CACHE:
        _CACHE[key] = _sim().simulate(*_inputs(name), CASES[name]["taps"], max_order=CASES[name]["max_order"])
    return _CACHE[key]


def _packed(name):
    rows, lead = R.rirs_of(CASES[name])
    return np.stack([np.concatenate([room, beta, src, lis, [yaw]]) for room, beta, src, lis, yaw, _, _ in rows]), lead


def test_tile_is_the_kernels():
    assert ops.ROOM_TILE == R.TILE and M.MAX_TAPS == R.MAX_TAPS
    assert (M.RATE, M.C, M.HEAD_RADIUS, M.HALF_WIDTH, M.EAR_PATTERN) == (R.RATE, R.C, R.HEAD_RADIUS, R.HALF_WIDTH, R.EAR_PATTERN)


@pytest.mark.parametrize("name", NAMES)
def test_cases_inside_the_bound(name):
    c = CASES[name]
    taps, order = c["taps"], c["max_order"]
    params, lead = _packed(name)
    Q, pad = params.shape[0], 1000
    pbuf = torch.full((pad + params.size + pad,), float("nan"), device=DEV, dtype=torch.float64)
    pbuf[pad:pad + params.size] = torch.from_numpy(params.reshape(-1)).to(DEV)
    obuf = torch.full((pad + Q * taps * 2 + pad,), float("nan"), device=DEV, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.m2h_room_sim(ctypes.c_void_p(pbuf.data_ptr() + 8 * pad), ctypes.c_void_p(obuf.data_ptr() + 4 * pad), Q, taps,
                                -1 if order is None else order, ops._stream(pbuf)), "m2h_room_sim")
    assert ops.last_kernel() == "room_sim"
    got = obuf.cpu().numpy()
    assert np.isnan(got[:pad]).all() and np.isnan(got[-pad:]).all()
    got = got[pad:-pad].reshape(Q, taps, 2)
    assert not np.isnan(got).any()
    h, s = R.reference(name)
    worst = max(R.ratio(got[q], h[q], s[q]) for q in range(Q))
    print("%-26s Q %2d taps %6d  worst |g - r| / s %.3e of tau %.3e" % (name, Q, taps, worst, R.TAU))
    assert worst <= R.TAU, (name, worst, R.TAU)
    out = _simulate(name)                                                       # the wrapper on views: the same bits, the stated layout
    assert out.shape == lead + (taps, 2) and out.dtype == torch.float32 and out.is_contiguous()
    assert np.array_equal(out.cpu().numpy().reshape(Q, taps, 2), got)
    if name == "taps700":
        assert (s[2:4] == 0).any() and np.array_equal(got[2:4] == 0, s[2:4] == 0)      # beta = 0: nothing but the direct sound


def test_float32_inputs_are_widened_exactly():
    a32 = _inputs("taps700", torch.float32)
    a64 = [t.to(torch.float64) for t in a32]
    x, y = _sim().simulate(*a32, 700), _sim().simulate(*a64, 700)
    assert x.shape == (3, 2, 700, 2) and torch.equal(x, y) and not torch.isnan(x).any()


def test_equal_bits_twice_solo_and_in_chunks_of_five():
    batch = _simulate("moving")
    assert torch.equal(_simulate("moving", _sim()), batch)
    assert torch.equal(_simulate("moving", M.RoomSimulator(DEV, chunk=5)), batch)
    room, beta, src, lis, yaw = _inputs("moving")
    for r, s, k in ((0, 0, 0), (1, 0, 2), (1, 1, 1)):
        solo = _sim().simulate(room[r:r + 1], beta[r:r + 1], src[r:r + 1, s:s + 1], lis[r:r + 1, k:k + 1], yaw[r:r + 1, k:k + 1], 3200)
        assert solo.shape == (1, 1, 1, 3200, 2) and torch.equal(solo[0, 0, 0], batch[r, s, k]), (r, s, k)
        still = _sim().simulate(room[r:r + 1], beta[r:r + 1], src[r:r + 1, s:s + 1], lis[r:r + 1, k], yaw[r:r + 1, k], 3200)     # no K axis
        assert still.shape == (1, 1, 3200, 2) and torch.equal(still[0, 0], batch[r, s, k])


def test_no_host_synchronisation_and_validate():
    args = _inputs("taps700")
    want = _simulate("taps700")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _sim().simulate(*args, 700)
        beta = M.beta_from_t60(args[0], 0.3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, want)
    want_beta = np.stack([R.beta_from_t60(r, 0.3) for r in CASES["taps700"]["room"]])
    assert beta.shape == (3, 6) and np.allclose(beta.cpu().numpy(), want_beta, rtol=1e-14, atol=0)
    assert torch.equal(_sim().simulate(*args, 700, validate=True), want)
    src = args[2].clone()
    src[1, 0, 1] = 3.2                                                          # room 1 is 3.1 m along y
    with pytest.raises(ValueError) as e:
        _sim().simulate(args[0], args[1], src, args[3], args[4], 700, validate=True)
    assert "inside their room" in str(e.value)
    out = _sim().simulate(args[0], args[1], src, args[3], args[4], 700)         # unchecked: that RIR is NaN, the others keep their bits
    assert torch.isnan(out[1, 0]).all() and torch.equal(out[0], want[0]) and torch.equal(out[1, 1], want[1, 1]) and torch.equal(out[2], want[2])


def test_the_moving_rirs_go_into_the_auralizer_and_roomacoustics_unchanged():
    from m2h.audio.acoustics import RoomAcoustics
    from m2h.audio.render import Auralizer
    rirs = _simulate("moving")
    g = torch.Generator().manual_seed(3)
    sources = (torch.rand(2, 2, 40000, generator=g) - 0.5).to(DEV)
    mix = Auralizer(DEV).render(sources, rirs)
    assert mix.shape == (2, 2, 40000) and torch.isfinite(mix).all() and float(mix.abs().max()) > 0
    out = RoomAcoustics(DEV).analyze(rirs)
    assert out["onset"].shape == (2, 2, 3) and out["peak"].shape == (2, 2, 3, 2) and out["params"].shape == (2, 2, 3, 2, 7, 7)
    h, _ = R.reference("moving")
    onset, peak = out["onset"].cpu().numpy().reshape(-1), out["peak"].cpu().numpy().reshape(-1, 2)
    for q in range(h.shape[0]):
        n0, npk, _, _ = AR.onset_f64(h[q].astype(np.float32))
        assert onset[q] == n0 and peak[q].tolist() == list(npk), (q, onset[q], peak[q], n0, npk)


def test_simulate_cli_writes_what_render_and_rir_read(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "a_rir.wav")
    r = subprocess.run([sys.executable, os.path.join(root, "simulate.py"), "--room", "5", "4", "3", "--beta", "0.9", "0.85", "0.8", "0.9", "0.7", "0.6",
                        "--source", "1", "2", "1.5", "--listener", "3", "2", "1.5", "--yaw", "0", "--seconds", "0.04375", "--out", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "700 taps" in r.stdout, r.stdout
    sys.path.insert(0, root)
    import render
    import rir
    h = rir.read_rir(out)
    h2, dtype = render.read_wav(out, 2)
    assert h.shape == (700, 2) and h.dtype == np.float32 and dtype == np.float32 and np.array_equal(h, h2)
    assert np.array_equal(h, _simulate("taps700")[0, 0].cpu().numpy())          # the same room, source, listener and yaw
