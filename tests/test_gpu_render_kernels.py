"""GPU: the Auralizer's kernels (csrc/render.hip: render_spectra, render_frames, render_mix) on every row of tests/render_kernels.py's table
through the C entry point m2h/audio/render.py itself calls, and Auralizer.render end to end on the chain rows; every element of every output
buffer against the float64 reference of the same float32 inputs: |g_e - r_e| <= tau * s_e (scales, kinds, taus, the rows beyond the issue:
tests/render_kernels.py, pinned on the CPU by tests/test_render_kernels_cpu.py together with the mutants the bound must reject).  Every
output buffer is NaN before the call: what a kernel must not write is still NaN afterwards, and what its window does not make it read is NaN
in its inputs.  No element is left out: the compared count is asserted to be the size of the whole buffer.  Every kernel call is one launch
with the kernel's own label.

Worst |g - r| / s per (family, kind) -- the float32 numpy restatement's over the rows (CPU), the MI355X's (test_zz_report_worst_ratios
prints them with -s), and the tau the kernel is held to, 8 x the ceiling the CPU test holds the restatement under:
  family   kind      restatement   MI355X      tau
  spectra  noise     6.46e-7       6.32e-7    5.6e-6
  spectra  impulse   4.54e-7       3.90e-7    4.0e-6
  spectra  dc        1.04e-5       1.04e-5    9.6e-5
  frames   noise     3.00e-6       3.00e-6    2.8e-5
  frames   impulse   8.95e-6       8.95e-6    8.0e-5
  mix      images    exact         exact
  mix      mix       2.81e-7       2.81e-7    TAU_FP32 = 2e-5
  chain    noise     1.52e-6       1.56e-6    1.44e-5
  chain    dc        6.49e-7       5.69e-7    6.4e-6
The MI355X follows the restatement: the frames and mix figures are the restatement's to three digits (the same products, the same
butterflies in the same order), the spectra's and the DC-heavy chain's lie a little under it, and the chain's 1.56e-6 is 3 % above its
restatement's 1.52e-6 and inside the ceiling of 1.8e-6 the restatement is held under.  No row found a kernel defect.  The 72 tests of this
file take 4 s on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

import render_kernels as Rk
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
WORST = {}
LABEL = {"spectra": "render_spectra", "frames": "render_frames", "mix": "render_mix"}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=_dev())


def _ids(family):
    return [r["id"] for r in Rk.ROWS[family]]


@pytest.fixture(scope="module")
def tw():
    from m2h.audio.twiddles import device_twiddles
    return device_twiddles(_dev())


def _one_launch(family, call):
    """Runs the entry point: one launch, labelled as the kernel."""
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    _lib.check(call(lib), "m2h_" + LABEL[family])
    assert ops.last_kernel() == LABEL[family] and lib.m2h_launch_count() == n0 + 1
    torch.cuda.synchronize()


def _check(row, name, g, r, s):
    """One output against (r, s), each kind's elements against its own tau; prints the figures before it asserts.  -> elements compared"""
    g = g.detach().cpu().numpy() if torch.is_tensor(g) else g
    assert g.shape == r.shape, (row["id"], name, g.shape, r.shape)
    total, bad = 0, []
    for kind, (worst, scale, ok, count) in Rk.compare(row, name, g, r, s).items():
        key = (row["family"], kind, name)
        WORST[key] = max(WORST.get(key, 0.0), worst)
        print("%-60s %-7s %-8s worst |g-r|/s %.2e of tau %.2e  scale-1 %+.1e  elements %d" % (row["id"], name, kind, worst, Rk.tau_of(row["family"], kind), scale - 1.0,
                                                                                              count))
        total += count
        if not ok:
            bad.append((kind, worst, scale))
    assert total == g.size == np.size(r), (row["id"], name, total, g.size)      # no element is left out
    assert not bad, (row["id"], name, bad)
    return total


@pytest.mark.parametrize("row_id", _ids("spectra"))
def test_render_spectra_matches_fp64(row_id, tw):
    row = Rk.ROWS_BY_ID[row_id]
    inp = Rk.inputs(row)
    x = _d(inp["x"])
    off, args = Rk.spectra_args(row)
    (gx, gy, gz), _ = Rk.spectra_grid(row)
    spec = _nan(gz, gy, gx, Rk.M, 2)
    base = ctypes.c_void_p(x.data_ptr() + 4 * off)                      # the base pointer moved to k0, as Auralizer.render's rir_spectra does
    _one_launch("spectra", lambda lib: lib.m2h_render_spectra(base, ops._ptr(tw), ops._ptr(spec), *args, ops._stream(x)))
    r, s = Rk.reference(row, inp)["spec"]
    assert _check(row, "spec", spec, r, s) == gz * gy * gx * Rk.M * 2
    assert np.array_equal(x.cpu().numpy(), inp["x"], equal_nan=True)


@pytest.mark.parametrize("row_id", _ids("frames"))
def test_render_frames_matches_fp64(row_id, tw):
    row = Rk.ROWS_BY_ID[row_id]
    inp = Rk.inputs(row)
    xs, hs = _d(inp["xspec"]), _d(inp["hspec"])
    frames = _nan(row["RS"], row["nm"], 2, Rk.FRAME)
    args = tuple(row[k] for k in ("RS", "J", "Pn", "K", "m0", "nm", "jx0", "nx", "kh0", "nh"))
    _one_launch("frames", lambda lib: lib.m2h_render_frames(ops._ptr(xs), ops._ptr(hs), ops._ptr(tw), ops._ptr(frames), *args, ops._stream(xs)))
    r, s = Rk.reference(row, inp)["frames"]
    assert _check(row, "frames", frames, r, s) == row["RS"] * row["nm"] * 2 * Rk.FRAME


@pytest.mark.parametrize("row_id", _ids("mix"))
def test_render_mix_matches_fp64(row_id):
    row = Rk.ROWS_BY_ID[row_id]
    inp = Rk.inputs(row)
    R, S, L = row["R"], row["S"], row["L_out"]
    fr, gains = _d(inp["frames"]), _d(inp["gains"])
    mix = _nan(R, 2, L)
    images = _nan(R, S, 2, L) if row["images"] else None
    args = tuple(row[k] for k in ("R", "S", "m0", "nm", "F", "o0", "o1", "L_out"))
    _one_launch("mix", lambda lib: lib.m2h_render_mix(ops._ptr(fr), ops._ptr(gains), ops._ptr(mix), ops._ptr(images), *args, ops._stream(fr)))
    ref = Rk.reference(row, inp)
    assert _check(row, "mix", mix, *ref["mix"]) == R * 2 * L
    if images is not None:
        assert _check(row, "images", images, *ref["images"]) == R * S * 2 * L
    _, _, n0, n1 = Rk.mix_window(row)
    g = mix.cpu().numpy()
    assert np.isfinite(g[..., n0:n1]).all() and np.isnan(g[..., :n0]).all() and np.isnan(g[..., n1:]).all()


@pytest.mark.parametrize("row_id", _ids("chain"))
def test_auralizer_render_matches_fp64_block_by_block(row_id):
    from m2h.audio.render import Auralizer
    row = Rk.ROWS_BY_ID[row_id]
    inp = Rk.inputs(row)
    x, h, gains = _d(inp["sources"]), _d(inp["rirs"] if row["K"] > 1 else inp["rirs"][:, :, 0]), _d(inp["gains"])
    mix, images = Auralizer(_dev(), max_blocks=row["max_blocks"]).render(x, h, gains=gains, tail=row["tail"], return_images=True)
    assert ops.last_kernel() == "render_mix"
    torch.cuda.synchronize()
    ref = Rk.reference(row, inp)
    assert _check(row, "images", images, *ref["images"]) == images.numel() and _check(row, "mix", mix, *ref["mix"]) == mix.numel()


def test_zz_report_worst_ratios():
    for (family, kind, name), v in sorted(WORST.items()):
        print("worst |g - r| / s  %-8s %-8s %-7s %.2e   restatement's ceiling %.2e   tau %.2e" % (family, kind, name, v, Rk.RESTATEMENT_WORST[(family, kind)],
                                                                                                  Rk.tau_of(family, kind)))
