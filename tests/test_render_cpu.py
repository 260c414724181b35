"""CPU: the Auralizer's plan and algorithm (m2h.audio.render, csrc/render.hip) against its definition, in float64.

The partitioned algorithm equals the definition to 1e-12 for every case of the GPU test and every chunking; the chunk plan covers
every output block once, computes every frame it reads and needs scratch that does not grow with the recording; the GPU test's bound
rejects four wrong renderers and accepts the same algorithm in fp32; the C entry points refuse bad arguments without a launch.
"""
import numpy as np
import pytest

import render_ref as REF
from m2h import _lib
from m2h.audio.render import BLOCK, MAX_PARTITIONS, chunk_scratch_bytes, render_plan

_refs = {}


def reference(case):
    """(sources, rirs, mix, images) of a case; the definition is evaluated once and shared"""
    if case not in _refs:
        x, h = REF.make_case(case)
        _refs[case] = (x, h) + REF.render_f64(x, h, tail=case[4])
        for a in _refs[case]:
            a.setflags(write=False)
    return _refs[case]


@pytest.mark.parametrize("case", REF.CASES, ids=REF.case_id)
def test_partitioned_algorithm_equals_the_definition(case):
    x, h, mix, images = reference(case)
    for max_blocks in (1, 2, 1024):
        got_mix, got_images = REF.render_partitioned_f64(x, h, tail=case[4], max_blocks=max_blocks)
        assert got_images.shape == images.shape and got_mix.shape == mix.shape
        e_img, e_mix = REF.rel_l1(got_images, images), REF.rel_l1(got_mix, mix)
        assert e_img < 1e-12 and e_mix < 1e-12, (max_blocks, e_img, e_mix)
        assert np.abs(got_images - images).max() <= 1e-12 * np.abs(images).max()


def test_static_scene_is_the_whole_signal_convolution():
    x, h = REF.make_sources(1, 2, 40001, 3), REF.make_rirs(1, 2, 1, 20000, 3)
    mix, images = REF.render_f64(x, h, tail=True)
    for s in range(2):
        for e in range(2):
            want = np.convolve(x[0, s].astype(np.float64), h[0, s, 0, :, e].astype(np.float64))
            assert np.abs(images[0, s, e] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.allclose(mix, 0.5 * (images[:, 0] + images[:, 1]), rtol=0, atol=1e-15)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("L,Lr", [(1, 1), (15999, 700), (16000, 16000), (16001, 16001), (40001, 33000), (16000 * 37 + 5, 48001), (16000 * 9, 256000)])
def test_plan_invariants(L, Lr, tail):
    J, Pn = -(-L // BLOCK), -(-Lr // BLOCK)
    for K in {1, J}:
        for max_blocks in (1, 2, 3, 7, 1024):
            plan = render_plan(L, Lr, K, max_blocks, tail)
            F = J + Pn - 1
            assert (plan["J"], plan["Pn"], plan["frames"]) == (J, Pn, F)
            assert plan["L_out"] == (L + Lr - 1 if tail else L) and plan["out_blocks"] == -(-plan["L_out"] // BLOCK) <= F + 1
            covered = []
            for ch in plan["chunks"]:
                (o0, o1), (m0, m1), (j0, j1), (k0, k1) = ch["out"], ch["frames"], ch["x"], ch["h"]
                assert 0 < o1 - o0 <= max_blocks and 0 < m1 - m0 <= max_blocks + 1 and 0 <= m0 and m1 <= F
                covered += range(o0, o1)
                for o in range(o0, o1):                                  # every frame the chunk's output reads is computed in it
                    for m in (o - 1, o):
                        assert not 0 <= m < F or m0 <= m < m1
                for m in range(m0, m1):                                  # every spectrum a frame reads is resident
                    for p in range(Pn):
                        if 0 <= m - p < J:
                            assert j0 <= m - p < j1 and (k0, k1) == ((0, 1) if K == 1 else (j0, j1))
                assert 0 <= j0 < j1 <= J and j1 - j0 <= max_blocks + Pn
            assert covered == list(range(plan["out_blocks"]))           # every output block exactly once, in order


def test_chunk_scratch_does_not_grow_with_the_recording():
    for K_moving in (False, True):
        for Lr in (8000, 48000):
            for max_blocks in (4, 64):
                peak = []
                for seconds in (300, 1000, 10000):                   # all longer than two chunks: each has a chunk with a frame before it
                    L = seconds * BLOCK - 3
                    plan = render_plan(L, Lr, -(-L // BLOCK) if K_moving else 1, max_blocks)
                    peak.append(max(chunk_scratch_bytes(plan, ch, 6, plan["J"] if K_moving else 1) for ch in plan["chunks"]))
                assert peak[0] == peak[1] == peak[2]
                Pn = -(-Lr // BLOCK)
                assert peak[0] <= 4 * 6 * ((max_blocks + 1) * 64000 + (max_blocks + Pn) * 32768 * (1 + (2 * Pn if K_moving else 0)) + 2 * Pn * 32768)


def test_plan_argument_errors():
    with pytest.raises(ValueError, match="K = 2"):
        render_plan(40001, 100, 2, 8)
    with pytest.raises(ValueError, match="limit is %d partitions" % MAX_PARTITIONS):
        render_plan(16000, 256001, 1, 8)
    assert render_plan(16000, 256000, 1, 8)["Pn"] == MAX_PARTITIONS
    for bad in ((0, 5, 1, 8), (5, 0, 1, 8), (5, 5, 1, 0)):
        with pytest.raises(ValueError):
            render_plan(*bad)


DEFECT_CASE = (2, 40001, 16001, 3, False)


def test_the_gpu_bound_rejects_wrong_renderers_and_accepts_fp32_arithmetic():
    """L = 40001, Lr = 16001, K = 3, the inputs of render_ref.  Measured, rel-L1 of the images: last partition dropped (it holds one
    tap) 3.2e-4, blocks after the first one sample late 0.82, the next second's RIR 1.3, the tail not carried across a block border 0.21;
    the algorithm on scipy's fp32 FFT 1.7e-7 .. 2.7e-7 over the GPU cases that fill a block (2.2e-8 for the one-sample case): the bound,
    2e-5, sits about 75x above the arithmetic and 16x below the smallest defect.  The fp32 restatement's largest element error is
    about 1/100 of the element-wise bound."""
    x, h, mix, images = reference(DEFECT_CASE)
    for defect in REF.DEFECTS:
        bad_mix, bad_images = REF.render_f64(x, h, defect=defect)
        e_img, e_mix = REF.rel_l1(bad_images[..., :images.shape[-1]], images), REF.rel_l1(bad_mix[..., :mix.shape[-1]], mix)
        print("defect %-24s rel-L1 images %.3e mix %.3e" % (defect, e_img, e_mix))
        assert e_img > REF.REL_L1_BOUND and e_mix > REF.REL_L1_BOUND, (defect, e_img, e_mix)
    worst = 0.0
    for case in REF.CASES:
        x, h, mix, images = reference(case)
        got_mix, got_images = REF.render_partitioned_f64(x, h, tail=case[4], max_blocks=2, dtype=np.float32)
        assert got_images.dtype == np.float32
        e_img, e_mix = REF.rel_l1(got_images, images), REF.rel_l1(got_mix, mix)
        T = REF.product_max(x, h)
        Pn = -(-case[2] // BLOCK)
        d = np.abs(got_images - images).max()
        print("fp32 %-28s rel-L1 images %.3e mix %.3e  max-abs %.3e of bound %.3e" % (REF.case_id(case), e_img, e_mix, d, REF.PRODUCT_BOUND * 2 * Pn * T))
        assert e_img < REF.REL_L1_BOUND / 20 and e_mix < REF.REL_L1_BOUND / 20
        assert d <= REF.PRODUCT_BOUND * 2 * Pn * T
        worst = max(worst, e_img, e_mix)
    assert worst < 1e-6


def test_entry_points_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    p = 4096   # any non-null, 16-byte aligned value: never dereferenced on a rejected call
    cases = [
        # x, twiddles, spec, n_outer, n_mid, n_inner, outer_stride, mid_stride, inner_stride, row_len, elem_stride, first_block, nblk, stream
        ("m2h_render_spectra", (None, p, p, 1, 1, 1, 16000, 0, 0, 16000, 1, 0, 1, None), b"render_spectra: null"),
        ("m2h_render_spectra", (p, p, None, 1, 1, 1, 16000, 0, 0, 16000, 1, 0, 1, None), b"render_spectra: null"),
        ("m2h_render_spectra", (p, p, p, 0, 1, 1, 16000, 0, 0, 16000, 1, 0, 1, None), b"render_spectra: bad sizes"),
        ("m2h_render_spectra", (p, p, p, 1, 1, 0, 16000, 0, 0, 16000, 1, 0, 1, None), b"render_spectra: bad sizes"),
        ("m2h_render_spectra", (p, p, p, 1, 1, 1, 16000, 0, 0, 0, 1, 0, 1, None), b"render_spectra: bad sizes"),
        ("m2h_render_spectra", (p, p, p, 1, 1, 1, 16000, 0, 0, 16000, 3, 0, 1, None), b"render_spectra: bad sizes"),
        ("m2h_render_spectra", (p, p, p, 1, 1, 1, 16000, 0, 0, 16000, 1, 0, 2, None), b"render_spectra: window"),       # the second block starts at the row's end
        ("m2h_render_spectra", (p, p, p, 1, 1, 1, 16000, 0, 0, 16001, 1, -1, 2, None), b"render_spectra: window"),
        # xspec, hspec, twiddles, frames, RS, J, Pn, K, m0, nm, jx0, nx, kh0, nh, stream
        ("m2h_render_frames", (p, None, p, p, 1, 3, 2, 1, 0, 4, 0, 3, 0, 1, None), b"render_frames: null"),
        ("m2h_render_frames", (p, p, p, p, 0, 3, 2, 1, 0, 4, 0, 3, 0, 1, None), b"render_frames: bad sizes"),
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 1, 0, 0, 0, 3, 0, 1, None), b"render_frames: bad sizes"),
        ("m2h_render_frames", (p, p, p, p, 1, 3, 17, 1, 0, 4, 0, 3, 0, 1, None), b"the limit is 16"),
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 2, 0, 4, 0, 3, 0, 2, None), b"render_frames: K = 2"),
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 1, 0, 5, 0, 3, 0, 1, None), b"render_frames: window: frames"),           # 5 frames of 4
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 1, 1, 3, 1, 2, 0, 1, None), b"render_frames: window: the frames read source blocks"),   # frame 1 reads block 0
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 1, 0, 4, 0, 2, 0, 1, None), b"render_frames: window: the frames read source blocks"),
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 3, 0, 4, 0, 3, 0, 2, None), b"render_frames: window: the frames read RIRs"),
        ("m2h_render_frames", (p, p, p, p, 1, 3, 2, 1, 0, 4, 0, 3, 0, 2, None), b"render_frames: window: a static scene"),
        ("m2h_render_frames", (p, p, p, p + 8, 1, 3, 2, 1, 0, 4, 0, 3, 0, 1, None), b"render_frames: buffers"),
        # frames, gains, mix, images, R, S, m0, nm, F, o0, o1, L_out, stream
        ("m2h_render_mix", (p, p, None, None, 1, 2, 0, 4, 4, 0, 3, 40001, None), b"render_mix: null"),
        ("m2h_render_mix", (p, None, p, None, 1, 2, 0, 4, 4, 0, 3, 40001, None), b"render_mix: null"),
        ("m2h_render_mix", (p, p, p, None, 1, 0, 0, 4, 4, 0, 3, 40001, None), b"render_mix: bad sizes"),
        ("m2h_render_mix", (p, p, p, None, 1, 2, 0, 4, 4, 0, 3, 0, None), b"render_mix: bad sizes"),
        ("m2h_render_mix", (p, p, p, None, 1, 2, 0, 4, 4, 0, 4, 40001, None), b"render_mix: window: output blocks"),        # block 3 starts past L_out
        ("m2h_render_mix", (p, p, p, None, 1, 2, 0, 4, 4, 3, 3, 80000, None), b"render_mix: window: output blocks"),
        ("m2h_render_mix", (p, p, p, None, 1, 2, 1, 3, 4, 1, 3, 40001, None), b"render_mix: window: the blocks read frames"),   # block 1 reads frame 0
        ("m2h_render_mix", (p, p, p, None, 1, 2, 0, 2, 4, 0, 3, 40001, None), b"render_mix: window: the blocks read frames"),
        ("m2h_render_mix", (p + 4, p, p, None, 1, 2, 0, 4, 4, 0, 3, 40001, None), b"render_mix: buffers"),
    ]
    for name, args, msg in cases:
        assert getattr(lib, name)(*args) < 0, (name, args)
        assert msg in lib.m2h_last_error(), (name, args, lib.m2h_last_error())
    assert lib.m2h_launch_count() == n0
