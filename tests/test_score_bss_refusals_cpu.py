"""Refusals of the BSS entry points (include/m2h.h, csrc/score_bss.hip), without a GPU: every refusal returns a negative status before any
HIP call, names the entry that was called, and launches nothing."""
import ctypes

import pytest

from m2h import _lib

P, NULL, ODD = ctypes.c_void_p(256), None, ctypes.c_void_p(260)      # never dereferenced

SHARED = [(dict(refs=NULL), b"null pointer"), (dict(est=NULL), b"null pointer"), (dict(mix=NULL), b"null pointer"), (dict(out=NULL), b"null pointer"),
          (dict(S=0), b"S = 0"), (dict(S=7), b"S = 7"), (dict(C=0), b"C = 0"), (dict(C=3), b"C = 3"), (dict(R=0), b"R = 0"),
          (dict(L=0), b"L = 0 samples; at least 2 D + 1 = 1"), (dict(lag=P, D=50, L=100), b"L = 100 samples; at least 2 D + 1 = 101"),
          (dict(lag=P), b"a lag table needs D >= 1"), (dict(D=1), b"a null pointer needs D = 0"), (dict(lag=P, D=8193, L=10 ** 6), b"D = 8193"),
          (dict(D=-1), b"D = -1"), (dict(T=0), b"T = 0 taps; 1 .. 512"), (dict(T=513), b"T = 513 taps; 1 .. 512"), (dict(T=-4), b"T = -4"),
          (dict(out=ODD), b"out must be 8-byte aligned"), (dict(tile=0), b"tile = 0"), (dict(tile=-5), b"tile = -5"),
          (dict(tile=1, L=2 ** 31, R=1, C=1), b"exceed a grid of 2^31 - 1 workgroups"), (dict(tile=3, L=2 ** 31, R=2, C=2), b"exceed a grid of 2^31 - 1 workgroups")]


def refused(lib, name, call, rows):
    n0 = lib.m2h_launch_count()
    for kw, text in rows:
        assert call(**kw) < 0, kw
        msg = lib.m2h_last_error()
        assert msg.startswith(name + b": ") and text in msg, (kw, msg)
    assert lib.m2h_launch_count() == n0


def test_bss_corr_refusals_name_the_entry_point():
    lib = _lib.load()

    def call(refs=P, est=P, mix=P, out=P, R=2, S=3, C=1, L=2000, tile=500, T=64, lag=None, D=0):
        return lib.m2h_bss_corr(refs, 6000, 2000, 0, est, 2000, 0, mix, 4000, 2000, out, R, S, C, L, tile, T, lag, D, None)

    refused(lib, b"bss_corr", call, SHARED)


def test_bss_project_refusals_name_the_entry_point():
    lib = _lib.load()

    def call(refs=P, est=P, mix=P, target=None, target0=0, h=P, out=P, R=2, S=3, C=1, L=2000, tile=500, T=64, lag=None, D=0):
        return lib.m2h_bss_project(refs, 6000, 2000, 0, est, 2000, 0, mix, 4000, 2000, target, target0, h, out, R, S, C, L, tile, T, lag, D, None)

    refused(lib, b"bss_project", call, SHARED + [(dict(h=NULL), b"null pointer (h)"), (dict(h=ODD), b"h must be 8-byte aligned"),
                                                 (dict(target0=3), b"target = 3"), (dict(target0=-1), b"target = -1")])


@pytest.mark.parametrize("name", ["m2h_bss_corr", "m2h_bss_project"])
def test_the_entry_points_are_declared(name):
    import os
    assert name in _lib.SIGNATURES
    with open(os.path.join(_lib.INCLUDE, "m2h.h")) as f:
        assert ("int %s(" % name) in f.read()
