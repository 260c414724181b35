"""Refusals of the STOI entry points (include/m2h.h, csrc/score_stoi.hip) and of Scorer.score(..., stoi=True), without a GPU: every refusal
returns a negative status before any HIP call, names the entry that was called, and launches nothing."""
import ctypes

import pytest

from m2h import _lib


def test_stoi_resample_refusals_name_the_entry_point():
    lib = _lib.load()
    p, null = ctypes.c_void_p(256), None          # never dereferenced
    n0 = lib.m2h_launch_count()

    def call(refs=p, est=p, mix=p, target0=0, G=p, out=p, R=2, S=3, C=1, L=100, lag=None, D=0):
        return lib.m2h_stoi_resample(refs, 300, 100, 0, est, 100, 0, mix, 200, 100, None, target0, G, out, R, S, C, L, lag, D, None)

    rows = [(dict(refs=null), b"null pointer"), (dict(est=null), b"null pointer"), (dict(mix=null), b"null pointer"), (dict(out=null), b"null pointer"),
            (dict(G=null), b"null pointer (G)"), (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(C=0), b"C = 0"), (dict(C=3), b"C = 3"),
            (dict(R=0), b"R = 0"), (dict(R=32768), b"R = 32768"), (dict(L=0), b"L = 0 samples; at least 2 D + 1 = 1"),
            (dict(lag=p, D=50, L=100), b"L = 100 samples; at least 2 D + 1 = 101"), (dict(lag=p), b"a lag table needs D >= 1"),
            (dict(D=1), b"a null pointer needs D = 0"), (dict(lag=p, D=8193, L=10 ** 6), b"D = 8193"), (dict(target0=3), b"target = 3"),
            (dict(target0=-1), b"target = -1"), (dict(out=ctypes.c_void_p(258)), b"out must be 4-byte aligned"),
            (dict(L=2 ** 31 * 256 * 8 // 5 + 8), b"exceed a grid of 2^31 - 1 workgroups")]
    for kw, text in rows:
        assert call(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert msg.startswith(b"stoi_resample: ") and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_stoi_ranges_refusals_name_the_entry_point():
    lib = _lib.load()
    p, odd4, odd2 = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    n0 = lib.m2h_launch_count()
    names = ("x10", "window", "twiddles", "ranges", "energy", "list", "kept", "env", "dseg", "out")

    def call(ld=100, L10=100, NR=2, Ftot=10, RC=2, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        return lib.m2h_stoi_ranges(a["x10"], ld, L10, a["window"], a["twiddles"], a["ranges"], NR, Ftot, RC, a["energy"], a["list"], a["kept"], a["env"],
                                   a["dseg"], a["out"], None)

    rows = [(dict([(k, None)]), b"null pointer") for k in names]
    rows += [(dict([(k, odd4)]), b"must be 8-byte aligned") for k in ("energy", "env", "dseg", "out", "ranges")]
    rows += [(dict([(k, odd2)]), b"must be 4-byte aligned") for k in ("x10", "window", "list", "kept")] + [(dict(twiddles=odd4), b"twiddles 8-byte aligned")]
    rows += [(dict(RC=0), b"RC = 0"), (dict(RC=65536), b"RC = 65536"), (dict(NR=0), b"NR = 0"), (dict(L10=0), b"L10 = 0"), (dict(ld=99), b"rows 99 apart"),
             (dict(Ftot=0), b"Ftot = 0"), (dict(Ftot=2 ** 31), b"exceed a grid of 2^31 - 1 workgroups")]
    for kw, text in rows:
        assert call(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert msg.startswith(b"stoi_ranges: ") and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_scorer_refuses_another_tile_and_host_tensors_before_any_launch():
    import torch
    from m2h.audio import score as SC
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    scorer = SC.Scorer("cuda:0")                  # (constructing a Scorer touches no device)
    z = lambda *shape: torch.zeros(shape)         # noqa: E731
    ok = dict(estimate=z(2, 50), references=z(2, 3, 50), mixture=z(2, 2, 50))
    for tile in (7, 15999, 32000):
        with pytest.raises(ValueError, match="stoi=True needs tile = 16000 .*got %d" % tile):
            scorer.score(stoi=True, tile=tile, **ok)
    with pytest.raises(ValueError, match="estimate must live on cuda:0, got cpu; the scorer has no CPU path"):
        scorer.score(stoi=True, **ok)
    assert lib.m2h_launch_count() == n0
