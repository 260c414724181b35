"""GPU: the three kernels of csrc/rir_acoustics.hip against the float64 definition (tests/acoustics_ref.py) inside the element bounds that
tests/test_acoustics_cpu.py pins, m2h_rir_decay on bins of the test's own making, and RoomAcoustics.analyze end to end.

Shapes: Lr = 1; 700 (one silent RIR and one silent ear in the batch); 12256 + 2064 + 17 with a 300-sample silent lead (n0 > 0, two
segments, a partial last bin); 30001 with a leading shape [2, 2, 3]; one row of 256000.  Kernel inputs lie inside a buffer that holds NaN
wherever the call names nothing, outputs hold NaN before the call.  (-s prints every measured ratio.)"""
import ctypes

import numpy as np
import pytest
import torch

import acoustics_ref as R
from m2h import _lib, ops
from m2h.audio import acoustics as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_CACHE = {}


def _batches():
    """name -> RIRs [..., Lr, 2] fp32 (numpy)"""
    if "batches" not in _CACHE:
        _CACHE["batches"] = {k: v[0] for k, v in R.batches().items()}
    return _CACHE["batches"]


def _reference(name):
    """the float64 definition for every RIR of a batch, computed once"""
    if ("ref", name) not in _CACHE:
        h = _batches()[name]
        _CACHE[("ref", name)] = [R.analyze_f64(x) for x in h.reshape(-1, h.shape[-2], 2)]
    return _CACHE[("ref", name)]


def _room():
    if "room" not in _CACHE:
        _CACHE["room"] = A.RoomAcoustics(DEV)
    return _CACHE["room"]


def _analysis(name, **kw):
    key = ("out", name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        out = _room().analyze(torch.from_numpy(_batches()[name]).to(DEV), **kw)
        _CACHE[key] = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    return _CACHE[key]


def _nan(shape, dtype):
    if dtype == torch.int32:
        return torch.full(shape, -(1 << 30), device=DEV, dtype=dtype)
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


@pytest.mark.parametrize("name", ["Lr1", "Lr700", "two_segments_lead300", "Lr30001", "Lr256000"])
def test_kernels_meet_their_bounds(name):
    h = _batches()[name]
    h = h.reshape(-1, h.shape[-2], 2)
    Q, Lr = h.shape[:2]
    nbs = -(-Lr // 16)
    pad = 1000
    buf = _nan((pad + h.size + pad,), torch.float32)
    buf[pad:pad + h.size] = torch.from_numpy(h.reshape(-1)).to(DEV)
    rirs = ctypes.c_void_p(buf.data_ptr() + 4 * pad)
    onset, peak = _nan((Q,), torch.int32), _nan((Q, 2), torch.int32)
    sums, drr = _nan((Q, 2, 2), torch.float64), _nan((Q, 2), torch.float64)
    energy, iacf, iacc = _nan((Q, 2, 7, nbs), torch.float64), _nan((Q, 7, 35), torch.float64), _nan((Q, 7, 2), torch.float64)
    masks, tw = _room()._tables()
    lib, st = _lib.load(), ops._stream(buf)
    _lib.check(lib.m2h_rir_onset(rirs, ops._ptr(onset), ops._ptr(peak), ops._ptr(sums), ops._ptr(drr), Q, Lr, st), "m2h_rir_onset")
    _lib.check(lib.m2h_rir_band_energy(rirs, ops._ptr(onset), ops._ptr(sums), ops._ptr(masks), ops._ptr(tw), ops._ptr(energy), ops._ptr(iacf), ops._ptr(iacc), Q, Lr, st),
               "m2h_rir_band_energy")
    torch.cuda.synchronize()
    onset, peak, sums, drr, energy, iacf, iacc = (t.cpu().numpy() for t in (onset, peak, sums, drr, energy, iacf, iacc))
    worst = {"energy": 0.0, "iacf": 0.0, "drr_sums": 0.0}
    for q, ref in enumerate(_reference(name)):
        assert onset[q] == ref["onset"] and peak[q].tolist() == ref["peak"].tolist(), (q, onset[q], peak[q], ref["onset"], ref["peak"])
        assert not np.isnan(energy[q]).any() and not np.isnan(iacf[q]).any() and not np.isnan(sums[q]).any()
        r = {"energy": R.ratio(energy[q], ref["energy"], R.energy_scale(h[q], ref["onset"], ref["energy"])),
             "iacf": R.ratio(iacf[q], ref["iacf"], R.iacf_scale(ref["iacf"])),
             "drr_sums": R.ratio(sums[q], ref["sums"], ref["sums"])}
        for k, v in r.items():
            worst[k] = max(worst[k], v)
        assert np.array_equal(np.isnan(drr[q]), np.isnan(ref["drr"]))
        ok = np.isfinite(ref["drr"])
        assert np.array_equal(drr[q][~ok], ref["drr"][~ok], equal_nan=True) and np.allclose(drr[q][ok], ref["drr"][ok], rtol=0, atol=1e-9)
        mine = R.iacc_of(iacf[q])                                            # the kernel's own sums through the definition's last step
        assert np.array_equal(iacc[q][:, 1], mine[:, 1], equal_nan=True) and np.allclose(iacc[q][:, 0], mine[:, 0], rtol=1e-14, atol=0, equal_nan=True)
    for k, v in worst.items():
        print("%-22s %-9s worst ratio %.3e of tau %.3e" % (name, k, v, R.TAU[k]))
    for k, v in worst.items():
        assert v <= R.TAU[k], (name, k, v, R.TAU[k])


def test_decay_kernel_on_bins_of_the_tests_making():
    bound = 100 * R.DECAY_ULP_CHANGE
    for name, E in R.decay_cases().items():
        rows = np.stack([E, E[::-1].copy(), 3.0 * E])                       # (a rising row has no decay to fit: NaN or a negative time, as the algebra gives)
        out = _nan((3, 7), torch.float64)
        bins = torch.from_numpy(rows).to(DEV)
        _lib.check(_lib.load().m2h_rir_decay(ops._ptr(bins), ops._ptr(out), 3, rows.shape[1], ops._stream(bins)), "m2h_rir_decay")
        got = out.cpu().numpy()
        want = np.stack([R.decay_f64(r) for r in rows])
        dev = R.param_dev(got, want)
        print("decay %-16s worst deviation %.2e of %.2e   %s" % (name, dev.max(), bound, np.array2string(got[0], precision=6)))
        assert dev.max() <= bound, (name, dev, got, want)
        assert np.array_equal(ops.rir_decay(bins).cpu().numpy(), got, equal_nan=True)


@pytest.mark.parametrize("name", ["Lr700", "two_segments_lead300", "Lr30001", "Lr256000"])
def test_analyze_end_to_end(name):
    out, refs = _analysis(name), _reference(name)
    lead = _batches()[name].shape[:-2]
    assert out["params"].shape == lead + (2, 7, 7) and out["iacc"].shape == lead + (7, 2) and out["onset"].shape == lead and out["peak"].shape == lead + (2,)
    assert out["drr"].shape == lead + (2,) and "energy" not in out and out["band_centres"] == A.BAND_CENTRES
    assert out["onset"].dtype == np.int32 and out["peak"].dtype == np.int32 and out["params"].dtype == np.float64
    params, iacc = out["params"].reshape(-1, 2, 7, 7), out["iacc"].reshape(-1, 7, 2)
    want_p, want_i = np.stack([r["params"] for r in refs]), np.stack([r["iacc"] for r in refs])
    assert np.array_equal(out["onset"].reshape(-1), [r["onset"] for r in refs])
    dev = R.param_dev(params, want_p)
    assert np.array_equal(np.isnan(iacc), np.isnan(want_i))
    di = float(np.nanmax(np.abs(iacc - want_i)[..., 0]))
    print("%-22s %s  iacc %.2e" % (name, " ".join("%s %.2e/%.2e" % (k, d, 8 * R.E2E_WORST[k]) for k, d in zip(A.ACOUSTIC_ORDER, dev)), di))
    assert np.array_equal(iacc[..., 1], want_i[..., 1], equal_nan=True)
    assert all(d <= 8 * R.E2E_WORST[k] for k, d in zip(A.ACOUSTIC_ORDER, dev)) and di <= 8 * R.E2E_WORST["iacc"], (dev, di)
    if name == "Lr700":                                                      # the silent RIR and the RIR with a silent right ear
        assert out["onset"][1] == 0 and np.isnan(out["params"][1]).all() and np.isnan(out["drr"][1]).all() and np.isnan(out["iacc"][1]).all()
        assert np.isnan(out["params"][2, 1]).all() and np.isnan(out["drr"][2, 1]) and np.isfinite(out["drr"][2, 0]) and np.isfinite(out["params"][2, 0, :, 5:]).all()


def test_lr1():
    out = _analysis("Lr1")
    assert out["onset"].tolist() == [0] and out["peak"].tolist() == [[0, 0]] and (out["drr"] == np.inf).all()
    p = out["params"][0]
    assert np.isnan(p[..., :3]).all() and (p[..., 3:5] == np.inf).all() and (p[..., 5] == 1.0).all() and (p[..., 6] == 0.0005).all()
    want = R.analyze_f64(_batches()["Lr1"][0])
    assert np.allclose(out["iacc"][0], want["iacc"], rtol=1e-6, atol=0, equal_nan=True)


def test_each_rir_of_a_batch_equals_its_solo_analysis_and_return_energy_changes_no_bit():
    batch = _analysis("Lr30001")
    with_e = _analysis("Lr30001", return_energy=True)
    assert with_e["energy"].shape == (2, 2, 3, 2, 7, 1876)
    for k in ("onset", "peak", "drr", "params", "iacc"):
        assert np.array_equal(batch[k], with_e[k], equal_nan=True), k
    h = torch.from_numpy(_batches()["Lr30001"]).to(DEV)
    chunked = A.RoomAcoustics(DEV, max_bin_bytes=5 * 2 * 7 * 1876 * 8).analyze(h, return_energy=True)      # five RIRs per launch
    for ix in ((0, 0, 0), (1, 0, 2), (1, 1, 1)):
        solo = _room().analyze(h[ix], return_energy=True)
        for k in ("onset", "peak", "drr", "params", "iacc", "energy"):
            assert np.array_equal(solo[k].cpu().numpy(), with_e[k][ix], equal_nan=True), (ix, k)
    for k in ("onset", "peak", "drr", "params", "iacc", "energy"):
        assert np.array_equal(chunked[k].cpu().numpy(), with_e[k], equal_nan=True), k
    silent = _analysis("Lr700")
    solo = _room().analyze(torch.from_numpy(_batches()["Lr700"][2]).to(DEV))
    assert np.array_equal(solo["params"].cpu().numpy(), silent["params"][2], equal_nan=True)


def test_analyze_makes_no_host_synchronisation():
    ra = _room()
    h = torch.from_numpy(_batches()["Lr700"]).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ra.analyze(h, return_energy=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out["params"].cpu().numpy(), _analysis("Lr700")["params"], equal_nan=True)


def test_the_auralizers_rirs_go_in_unchanged():
    from m2h.audio.render import Auralizer
    g = torch.Generator().manual_seed(3)
    R_, S, K, Lr = 1, 2, 2, 700
    rirs = torch.from_numpy(np.stack([R.noise_rir(Lr, 0.04 + 0.01 * i, 40 + i) for i in range(R_ * S * K)]).reshape(R_, S, K, Lr, 2)).to(DEV)
    sources = (torch.rand(R_, S, 16001, generator=g) - 0.5).to(DEV)
    mix = Auralizer(DEV).render(sources, rirs)
    out = _room().analyze(rirs)
    assert mix.shape == (R_, 2, 16001) and out["params"].shape == (R_, S, K, 2, 7, 7) and out["iacc"].shape == (R_, S, K, 7, 2) and out["onset"].shape == (R_, S, K)
    flat = _room().analyze(rirs.reshape(-1, Lr, 2))
    assert np.array_equal(out["params"].cpu().numpy().reshape(-1, 2, 7, 7), flat["params"].cpu().numpy(), equal_nan=True)
    want = R.analyze_f64(rirs[0, 1, 1].cpu().numpy())
    assert int(out["onset"][0, 1, 1]) == want["onset"] and R.param_dev(out["params"][0, 1, 1].cpu().numpy(), want["params"]).max() <= 8 * max(R.E2E_WORST.values())
