"""GPU: rir_onset_kernel, rir_band_energy_kernel and rir_decay_kernel (csrc/rir_acoustics.hip) on every row of tests/acoustics_kernels.py's
tables through m2h_rir_onset, m2h_rir_band_energy and m2h_rir_decay themselves (rows, cells, kinds, taus, mutants: tests/acoustics_kernels.py,
pinned on the CPU by tests/test_acoustics_kernels_cpu.py).  An RIR lies inside NaN; every output is NaN (-(1 << 30) for the ints) before the
call and its pads are NaN afterwards; each call is one launch with its own label.  onset and peak must equal the definition's; sums, energy and
iacf are compared element by element against the definition, the count asserted; drr and iacc follow the definition's last step applied to
the kernel's own sums; zero-filled segments are exactly 0.0 in all 7 bands and both ears.  The decay rows lie inside NaN too and follow
acoustics_ref's rule, 100 x DECAY_ULP_CHANGE.

Worst ratio per kind -- the restatement's over the rows (CPU), the MI355X's (test_zz_report prints them with -s), and the tau, 8 x the ceiling
the CPU test holds the restatement under:
  kind        restatement   MI355X      tau
  energy      4.10e-7       7.57e-7     4.0e-6      (Lr24512 / threshold)
  iacf        3.17e-7       4.93e-7     2.56e-6     (tie.tree / Lr17)
  drr sums    4.42e-16      4.42e-16    4.0e-15     (tie.tree)
  decay       7.1e-15       7.1e-15     3.6e-13     (nb65.rows5; 100 x DECAY_ULP_CHANGE)
The restatement's transforms are scipy's in single precision, the kernel's its own radix passes: the energy and iacf figures differ by the
transforms' rounding, both well inside tau.  Every row reports its compared count as the whole buffer (energy 2 x 7 x ceil(Lr / 16), iacf
245, sums 4, decay 7 per row).  No row found a kernel defect.  The 40 tests of this file take 3.2 s on an MI355X.
"""
import numpy as np
import pytest
import torch

import acoustics_kernels as K
import acoustics_ref as R
from m2h import _lib, ops
from m2h.audio import acoustics as A

pytestmark = pytest.mark.gpu
WORST = {}
_CACHE = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _padded(shape, dtype):
    """(the whole buffer, the view of the inside): NaN (INT_FILL) everywhere, K.PAD elements either side"""
    n = int(np.prod(shape))
    fill = K.INT_FILL if dtype == torch.int32 else float("nan")
    buf = torch.full((K.PAD + n + K.PAD,), fill, device=_dev(), dtype=dtype)
    return buf, buf[K.PAD:K.PAD + n].view(shape)


def _untouched(buf):
    pads = torch.cat([buf[:K.PAD], buf[-K.PAD:]]).cpu().numpy()
    return bool((pads == K.INT_FILL).all()) if buf.dtype == torch.int32 else bool(np.isnan(pads).all())


def _one_launch(label, call):
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    _lib.check(call(lib), "m2h_" + label)
    assert ops.last_kernel() == label and lib.m2h_launch_count() == n0 + 1
    torch.cuda.synchronize()


def _note(kind, v, name):
    WORST[kind] = max(WORST.get(kind, (0.0, "")), (v, name))


@pytest.mark.parametrize("name", list(K.RIR_ROWS))
def test_onset_and_band_energy_match_fp64(name):
    h = K.RIR_ROWS[name]
    Lr = h.shape[0]
    nbs = -(-Lr // R.BIN)
    hbuf, hin = _padded((Lr, 2), torch.float32)
    hin.copy_(torch.from_numpy(h))
    (ob, onset), (pb, peak) = _padded((1,), torch.int32), _padded((1, 2), torch.int32)
    (sb, sums), (db, drr) = _padded((1, 2, 2), torch.float64), _padded((1, 2), torch.float64)
    (eb, energy), (fb, iacf), (cb, iacc) = _padded((1, 2, 7, nbs), torch.float64), _padded((1, 7, 35), torch.float64), _padded((1, 7, 2), torch.float64)
    if "tables" not in _CACHE:
        _CACHE["tables"] = A.RoomAcoustics(_dev())._tables()
    masks, tw = _CACHE["tables"]
    st = ops._stream(hbuf)
    _one_launch("rir_onset", lambda lib: lib.m2h_rir_onset(ops._ptr(hin), ops._ptr(onset), ops._ptr(peak), ops._ptr(sums), ops._ptr(drr), 1, Lr, st))
    _one_launch("rir_band_energy", lambda lib: lib.m2h_rir_band_energy(ops._ptr(hin), ops._ptr(onset), ops._ptr(sums), ops._ptr(masks), ops._ptr(tw), ops._ptr(energy),
                                                                       ops._ptr(iacf), ops._ptr(iacc), 1, Lr, st))
    assert all(_untouched(b) for b in (hbuf, ob, pb, sb, db, eb, fb, cb))     # nothing past nbs, nothing outside any output
    assert np.array_equal(hin.cpu().numpy(), h)
    onset, peak, sums, drr, energy, iacf, iacc = (t.cpu().numpy()[0] for t in (onset, peak, sums, drr, energy, iacf, iacc))
    ref = K.reference(name)
    assert onset == ref["onset"] and peak.tolist() == ref["peak"].tolist(), (name, onset, peak, ref["onset"], ref["peak"])
    assert not np.isnan(energy).any() and not np.isnan(iacf).any() and not np.isnan(sums).any()
    got = {"energy": R.ratio(energy, ref["energy"], R.energy_scale(h, ref["onset"], ref["energy"])), "iacf": R.ratio(iacf, ref["iacf"], R.iacf_scale(ref["iacf"])),
           "drr_sums": R.ratio(sums, ref["sums"], ref["sums"])}
    count = {"energy": energy.size, "iacf": iacf.size, "drr_sums": sums.size}
    assert count == {"energy": 2 * 7 * nbs, "iacf": 7 * 35, "drr_sums": 4} == {"energy": ref["energy"].size, "iacf": ref["iacf"].size, "drr_sums": ref["sums"].size}
    for k, v in got.items():
        print("%-20s %-9s worst ratio %.3e of tau %.3e  elements %d" % (name, k, v, K.TAU[k], count[k]))
        _note(k, v, name)
    zf, segs = K.zero_filled_segments(int(onset), Lr)
    for g in zf:
        assert (energy[:, :, R.SEG_BINS * g:R.SEG_BINS * (g + 1)] == 0.0).all(), (name, g)      # exactly 0.0, 7 bands, both ears
    assert np.array_equal(np.isnan(drr), np.isnan(ref["drr"]))
    ok = np.isfinite(ref["drr"])
    with np.errstate(divide="ignore", invalid="ignore"):
        mine = 10.0 * np.log10(sums[:, 0] / (sums[:, 1] - sums[:, 0]))     # the definition's last step on the kernel's own sums
    assert np.array_equal(drr[~ok], ref["drr"][~ok], equal_nan=True) and np.allclose(drr[ok], mine[ok], rtol=0, atol=1e-12)
    mine = R.iacc_of(iacf)
    assert np.array_equal(iacc[:, 1], mine[:, 1], equal_nan=True) and np.allclose(iacc[:, 0], mine[:, 0], rtol=1e-14, atol=0, equal_nan=True)
    for k, v in got.items():
        assert v <= K.TAU[k], (name, k, v, K.TAU[k])


@pytest.mark.parametrize("name", list(K.DECAY_TABLES))
def test_decay_kernel_matches_fp64(name):
    E = K.DECAY_TABLES[name]
    rows, nb = E.shape
    bbuf, bins = _padded((rows, nb), torch.float64)
    bins.copy_(torch.from_numpy(E))
    obuf, out = _padded((rows, 7), torch.float64)
    _one_launch("rir_decay", lambda lib: lib.m2h_rir_decay(ops._ptr(bins), ops._ptr(out), rows, nb, ops._stream(bbuf)))
    assert _untouched(obuf) and _untouched(bbuf)
    got = out.cpu().numpy()
    want = np.stack([R.decay_f64(r) for r in E])
    dev = R.param_dev(got, want)
    print("decay %-16s rows %d nb %5d  worst deviation %.2e of %.2e  elements %d" % (name, rows, nb, dev.max(), K.DECAY_BOUND, got.size))
    _note("decay", float(dev.max()), name)
    assert got.size == rows * 7 == want.size and dev.max() <= K.DECAY_BOUND, (name, dev, got, want)


def test_zz_report():
    for kind, (w, name) in sorted(WORST.items()):
        print("worst ratio  %-9s %.3e (%s)   restatement's ceiling %.3e   tau %.3e" % (kind, w, name, K.RESTATEMENT_WORST.get(kind, K.DECAY_RESTATEMENT_WORST),
                                                                                        K.TAU.get(kind, K.DECAY_BOUND)))
