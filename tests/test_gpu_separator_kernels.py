"""GPU: the kernels of the shipped path -- csrc/separate.hip (sep_frames, sep_stft_post, sep_istft_pre, sep_bin_rows, sep_istft_ola,
sep_istft_xfade, whole-recording and window forms), csrc/resample.hip (every tile size with one phase and with a table, the direct kernel,
whole rows and the window form) and the three slice kernels of csrc/layout.hip -- on every row of tests/separator_kernels.py's table through
the m2h.ops function the project itself calls (m2h_sep_frames and the split32 slice through the C ABI: ops does not reach them), every
element of every output buffer against the float64 reference of the same float32 inputs: |g_e - r_e| <= tau * s_e (scales, taus and the
departures from the issue: tests/separator_kernels.py, pinned on the CPU by tests/test_separator_kernels_cpu.py together with the mutants the
bound must reject).  Every output buffer is NaN before the call: what a kernel must not write is still NaN afterwards, what it must not use is
NaN in its inputs.  No element is left out: the compared count is asserted to be the size of the whole buffer, the floats around a view
included.

Worst |g - r| / s measured on an MI355X over each family's rows (test_zz_report_worst_ratios prints them with -s) beside the float32 numpy
restatement's, and the tau it is held to:
  frames     exact                                                    (restatement exact)
  post       log1p|X| 7.05e-8, phasor 1.26e-7                         (restatement 1.26e-7)     TAU_FP32 = 2e-5
  pre        1.53e-7                                                  (restatement 1.80e-7)     TAU_FP32
  bin_rows   exact                                                    (restatement exact)
  ola        1.25e-7                                                  (restatement 1.39e-7)     TAU_FP32
  xfade      1.20e-7                                                  (restatement 1.21e-7)     TAU_FP32
  resample   2.72e-6 (512000 -> 16000, T = 641)                       (restatement 2.72e-6)     TAU_FP32
             the 20001-tap chain of 1000 -> 1: 1.67e-5                (restatement 1.67e-5)     1.4e-4 = 8 x 1.75e-5
  slice      unmasked, plane and unmasked split32 exact; masked: generic 6.93e-8, tiled 1.35e-7 (restatement 1.4e-7), tiled split32
             3.48e-6 against s + 2^-17 |r|                            (restatement 3.34e-6)     TAU_FP32
No measured ratio exceeds its restatement's by more than 5 % (the 4x that would ask for a reason is far off); the resampler's are the
restatement's to three digits (the same fmaf chain).  At the 1e37 plants of post the kernel's magnitude is +inf (float32 re^2 + im^2), which
the reference accepts there beside the float64 value.  The 67 tests of this file take 6 s on an MI355X; no row found a kernel defect.
"""
import numpy as np
import pytest
import torch

import separator_kernels as Sk
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
WORST = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=_dev())


def _ids(family, pred=lambda r: True):
    return [r["id"] for r in Sk.ROWS[family] if pred(r)]


def _check(row, name, g, r, s, inf_ok=None, key=None):
    """One output against (r, s[, where +inf is accepted]); prints the figures before it asserts.  -> elements compared"""
    g = g.detach().cpu().numpy() if torch.is_tensor(g) else g
    worst, scale, ok, count = Sk.check(g, r, s, Sk.tau_of(row), inf_ok)
    key = key or (row["family"] + (" (long chain)" if Sk.tau_of(row) != Sk.TAU[row["family"]] else ""), name)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%-62s %-8s worst |g-r|/s %.2e  scale-1 %+.1e  elements %d" % (row["id"], name, worst, scale - 1.0, count))
    assert count == g.size == np.size(r), (row["id"], name, count, g.size, np.size(r))      # no element is left out
    assert ok, (row["id"], name, worst, scale)
    return count


def _blocks(row):
    step = Sk.OLA_BLOCK if Sk.is_big(row) else row["R"]
    return [slice(i, min(i + step, row["R"])) for i in range(0, row["R"], step)]


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", _ids("frames"))
def test_sep_frames_are_the_exact_windowed_segment_local_reflection(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    buf, w = _d(inp["buf"]), _d(inp["window"])
    R, nseg = row["R"], row["nseg"]
    out = _nan(nseg * R * 2 * Sk.SEP_T, Sk.SEP_LD)
    if row["entry"] == "m2h_sep_frames":
        assert row["hop"] == Sk.SEP_SEG and not row["win"]
        _lib.check(_lib.load().m2h_sep_frames(ops._ptr(buf), ops._ptr(w), ops._ptr(out), R, row["end"], row["s0"], nseg, ops._stream(buf)), "m2h_sep_frames")
        assert ops.last_kernel() == "sep_frames"
    elif row["win"]:
        assert ops.sep_frames(buf, w, row["s0"], nseg, hop=row["hop"], origin=row["origin"], end=row["end"], out=out) is out
        assert ops.last_kernel() == "sep_frames_win"
    else:
        assert ops.sep_frames(buf, w, row["s0"], nseg, hop=row["hop"], out=out) is out
        assert ops.last_kernel() == "sep_frames_hop"
    torch.cuda.synchronize()
    r, s = Sk.reference(row, inp)["frames"]
    assert _check(row, "frames", out, r, s) == nseg * R * 2 * Sk.SEP_T * Sk.SEP_LD


@pytest.mark.parametrize("row_id", _ids("post"))
def test_sep_stft_post_matches_fp64(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    mag, phasor = ops.sep_stft_post(_d(inp["spec"]), row["N"])
    assert ops.last_kernel() == "sep_stft_post"
    torch.cuda.synchronize()
    ref = Sk.reference(row, inp)
    zero = ref["phasor"][1][..., 0] == 0
    g = phasor.cpu().numpy()
    assert zero.sum() >= 2 * Sk.SEP_NB and (g[zero] == (1.0, 0.0)).all() and np.isfinite(g).all()      # np.angle(0) = 0, and no overflow at 1e37
    for name, t in (("mag", mag), ("phasor", phasor)):
        assert _check(row, name, t, *ref[name]) == row["N"] * Sk.SEP_NB * Sk.SEP_T * 2


@pytest.mark.parametrize("row_id", _ids("pre"))
def test_sep_istft_pre_matches_fp64(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    P, ph = _d(inp["P"]), _d(inp["phasor"])
    if row["out"]:
        out = _nan(row["N"] * Sk.SEP_T, Sk.SEP_LD)
        assert ops.sep_istft_pre(P, ph, out=out) is out
    else:
        out = ops.sep_istft_pre(P, ph)
    assert ops.last_kernel() == "sep_istft_pre"
    torch.cuda.synchronize()
    assert _check(row, "rows", out, *Sk.reference(row, inp)["rows"]) == row["N"] * Sk.SEP_T * Sk.SEP_LD


@pytest.mark.parametrize("row_id", _ids("bin_rows"))
def test_sep_bin_rows_is_the_exact_masked_spectrum(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    spec, masks = _d(inp["spec"]), _d(inp["masks"])
    if row["inplace"]:
        out = ops.sep_bin_rows(spec, masks)
        assert out is spec
    else:
        out = _nan(*spec.shape)
        assert ops.sep_bin_rows(spec, masks, out=out) is out and np.array_equal(spec.cpu().numpy(), inp["spec"])
    assert ops.last_kernel() == "sep_bin_rows"
    torch.cuda.synchronize()
    assert _check(row, "rows", out, *Sk.reference(row, inp)["rows"]) == row["N"] * 2 * Sk.SEP_T * Sk.SEP_LD


@pytest.mark.parametrize("row_id", _ids("ola"))
def test_sep_istft_ola_matches_fp64(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    R, cap = row["R"], row["cap"]
    w, y = _d(inp["window"]), _nan(R, cap)
    for (s0, nseg), fr in zip(row["calls"], inp["frames"]):
        fr = _d(fr.reshape(nseg * R * Sk.SEP_T, Sk.SEP_LD))
        if row["win"]:
            ops.sep_istft_ola(fr, w, y, s0, nseg, origin=row["origin"], end=row["end"])
            assert ops.last_kernel() == "sep_istft_ola_win"
        else:
            ops.sep_istft_ola(fr, w, y, s0, nseg)
            assert ops.last_kernel() == "sep_istft_ola"
    torch.cuda.synchronize()
    g = y.cpu().numpy()
    count = 0
    for rsel in _blocks(row):            # blocks of batch rows: host memory stays modest
        r, s = Sk.ola_reference(row, inp, rsel)["y"]
        count += _check(row, "y", g[rsel], r, s)
    assert count == R * cap


@pytest.mark.parametrize("row_id", _ids("xfade"))
def test_sep_istft_xfade_matches_fp64_call_by_call(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    R, cap, hop = row["R"], row["cap"], row["hop"]
    w, xw = _d(inp["window"]), _d(inp["xwin"])
    g = np.full((R, cap), np.nan, dtype=np.float32)
    for ci, (s0, nseg, origin, end) in enumerate(row["calls"]):
        prior = Sk.xf_prior(row, ci, g)                      # the float32 y this call is handed: what the previous call left, moved where the origin advanced
        y = _d(prior)
        fr = _d(inp["frames"][ci].reshape(nseg * R * Sk.SEP_T, Sk.SEP_LD))
        if row["win"]:
            ops.sep_istft_xfade(fr, w, xw, y, hop, s0, nseg, origin=origin, end=end)
            assert ops.last_kernel() == "sep_istft_xfade_win"
        else:
            ops.sep_istft_xfade(fr, w, xw, y, hop, s0, nseg)
            assert ops.last_kernel() == "sep_istft_xfade"
        torch.cuda.synchronize()
        g = y.cpu().numpy()
        count = 0
        for rsel in _blocks(row):
            r, s = Sk.xf_reference_call(row, inp, ci, prior[rsel], rsel)["y"]
            count += _check(row, "y call %d" % ci, g[rsel], r, s, key=("xfade", "y"))
        assert count == R * cap
    assert not np.isnan(g[:, :end - origin]).any() and np.isnan(g[:, end - origin:]).all()


@pytest.mark.parametrize("row_id", _ids("resample"))
def test_resample_matches_the_fp64_definition(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    rows, cap, count, xoff, yoff = (row[k] for k in ("rows", "cap", "count", "xoff", "yoff"))
    x_alloc, G = _d(inp["x_alloc"]), _d(inp["G"])
    y_alloc = _nan(yoff + rows * count + Sk.RS_PAD)
    x = x_alloc[xoff:xoff + rows * cap].view(rows, cap)        # views 0 .. 3 floats into their allocations
    y = y_alloc[yoff:yoff + rows * count].view(rows, count)
    assert x.data_ptr() % 16 == 4 * (xoff % 4) and y.data_ptr() % 16 == 4 * (yoff % 4)
    if row["win"]:
        ops.resample_poly(x, G, inp["up"], inp["down"], out=y, origin=row["origin"], end=row["end"], n_first=row["n_first"], count=count)
    else:
        ops.resample_poly(x, G, inp["up"], inp["down"], out=y)
    kernel, phases = Sk.rs_kernel(row)
    assert ops.last_kernel() == "resample_poly" + ("_win" if row["win"] else "") + ("_direct" if kernel == "direct" else "")
    torch.cuda.synchronize()
    r, s = Sk.reference(row, inp)["y"]
    assert _check(row, "y", y_alloc, r, s) == yoff + rows * count + Sk.RS_PAD
    assert np.array_equal(x_alloc.cpu().numpy(), inp["x_alloc"], equal_nan=True)


@pytest.mark.parametrize("row_id", _ids("slice"))
def test_sep_slice_input_matches_fp64(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    B, F, T, C = (row[k] for k in ("B", "F", "T", "C"))
    mix = _d(inp["mix"])
    masks = _d(inp["masks"]) if inp["masks"] is not None else None
    if row["form"] == "plane":
        out = ops.sep_slice_input_plane(mix, _d(inp["cls"]), ldo=row["ldo"])
        assert ops.last_kernel() == "sep_slice_input_plane" and tuple(out.shape) == (B, F // 16, T, row["ldo"])
    elif row["split"]:      # ops does not reach split_out: the C ABI, into a buffer of NaN
        out = _nan(B, F // 16, T, 16 * C)
        _lib.check(_lib.load().m2h_sep_slice_input_fmt(ops._ptr(mix), ops._ptr(masks), ops._ptr(out), B, F, T, C, 1, ops._stream(mix)), "m2h_sep_slice_input_fmt")
        assert ops.last_kernel() == "sep_slice_input"
    else:
        out = ops.sep_slice_input(mix, masks)
        assert ops.last_kernel() == "sep_slice_input" and tuple(out.shape) == (B, F // 16, T, 16 * C)
    torch.cuda.synchronize()
    g = out.cpu().numpy()
    if row["split"]:
        g = Sk.unsplit32(g)
    r, s = Sk.reference(row, inp)["out"]
    key = ("slice", "%s%s%s" % (Sk.sl_kernel(row), " masked" if masks is not None else "", " split32" if row["split"] else ""))
    assert _check(row, "out", g, r, s, key=key) == out.numel()
    if masks is not None and not row["split"]:      # exactly 0 where m (e - 1) <= 0
        off = Sk._sl_layout((inp["masks"] <= 0) | (inp["mix"] == 0))
        assert (g[off] == 0).all()


def test_zz_report_worst_ratios():
    for key, v in sorted(WORST.items()):
        print("worst |g - r| / s  %-28s %-8s %.2e" % (key[0], key[1], v))
