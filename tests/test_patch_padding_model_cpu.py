"""CPU model of the shared-patch engine's all-padding rule (csrc/conv_patch.hip, whole-image patch form): which (tap, pixel
fragment) pairs of a k-tile read nothing but zero rows, so that the kernel may leave their MFMAs out.

The kernel keeps one wave-uniform bit per (tap tt, fragment mi): set when the fragment's pixels lie on the image's top (bottom) row
and the tap reaches one row up (down) -- `(edge & kill & 3) != 0` on the wave's first lane -- and only for image rows of at least 16
pixels, where the 16 pixels of a fragment are (part of) ONE image row.  Here the rule is restated in numpy and checked against brute
force over the per-lane address-table rule (`edge & kill`, the formulas of build_atab), for every power-of-two pixel grid of both
tiles, conv classes and transposed-conv phases; and a float32 conv / transposed conv with the masked pairs left out must have the
bits of the one that multiplies the zeros."""
import itertools

import numpy as np
import pytest

TILES = {256: 4, 512: 8}   # pixel rows of a tile -> its waves along m (a wave: 64 pixels = four 16-pixel fragments)
GRIDS = [(1 << r, 1 << w) for r in range(10) for w in range(10) if (1 << r) * (1 << w) <= 512]   # (rows, W) of one image
ENABLED = [(2, 16), (4, 16), (2, 32)]   # the launcher's rule: W >= 16, rows >= 2, rows W <= 64 (whole images per wave), 256-row tile


def kill_of(tt, gh, gw):
    """Edges tap tt = 2 a + b of class / phase (gh, gw) reaches over: bit 0 top, 1 bottom, 2 left, 3 right (build_atab)."""
    a, b = tt >> 1, tt & 1
    return (1 if a == 0 and gh == 0 else 0) | (2 if a == 1 and gh == 1 else 0) | (4 if b == 0 and gw == 0 else 0) | (8 if b == 1 and gw == 1 else 0)


def edge_of(ml, rows, W):
    """Image edges pixel ml of the tile lies on (whole images per tile: pixel ml is pixel ml % (rows W) of image ml // (rows W))."""
    rem = ml % (rows * W)
    il, jl = rem // W, rem % W
    return (1 if il == 0 else 0) | (2 if il == rows - 1 else 0) | (4 if jl == 0 else 0) | (8 if jl == W - 1 else 0)


def dead_mask(rows, W, wm, gh, gw):
    """The kernel's rule: bit 4 tt + mi from the wave's FIRST lane, top / bottom reasons only, image rows of 16 pixels and more."""
    m = 0
    if W < 16:
        return 0
    for tt in range(4):
        for mi in range(4):
            if edge_of(wm * 64 + mi * 16, rows, W) & kill_of(tt, gh, gw) & 3:
                m |= 1 << (4 * tt + mi)
    return m


def all_lanes_read_zero_rows(rows, W, wm, tt, mi, gh, gw):
    """Brute force over the address-table rule: a lane reads the zero row iff edge & kill != 0 (any of the four reasons)."""
    return all(edge_of(wm * 64 + mi * 16 + frow, rows, W) & kill_of(tt, gh, gw) for frow in range(16))


def cases():
    for bm, waves in TILES.items():
        for rows, W in GRIDS:
            if rows * W <= bm:   # whole images per tile
                yield bm, waves, rows, W


def test_bit_is_set_iff_all_sixteen_lanes_read_zero_rows():
    n_set = 0
    for bm, waves, rows, W in cases():
        for gh, gw, wm in itertools.product(range(2), range(2), range(waves)):
            m = dead_mask(rows, W, wm, gh, gw)
            if W < 16:
                assert m == 0, (bm, rows, W)   # a fragment holds several image rows (top AND bottom ones): never
                continue
            for tt, mi in itertools.product(range(4), range(4)):
                bit = (m >> (4 * tt + mi)) & 1
                assert bit == all_lanes_read_zero_rows(rows, W, wm, tt, mi, gh, gw), (bm, rows, W, gh, gw, wm, tt, mi)
                n_set += bit
    assert n_set > 0


def test_narrow_images_have_fragments_with_top_and_bottom_rows():
    """Why W < 16 is excluded: 2 x 8 -- a fragment is a whole image, its lanes disagree about the top / bottom edge."""
    edges = {edge_of(frow, 2, 8) & 3 for frow in range(16)}
    assert edges == {1, 2}
    assert dead_mask(2, 8, 0, 0, 0) == 0


@pytest.mark.parametrize("rows,W", ENABLED)
def test_every_wave_has_the_same_number_of_dead_fragments_in_every_k_tile(rows, W):
    for gh, gw in itertools.product(range(2), range(2)):
        for tt in range(4):
            counts = {bin((dead_mask(rows, W, wm, gh, gw) >> (4 * tt)) & 15).count("1") for wm in range(TILES[256])}
            assert len(counts) == 1, (rows, W, gh, gw, tt, counts)


def test_enabled_grids_are_those_with_whole_images_per_wave():
    got = [(rows, W) for rows, W in GRIDS if W >= 16 and rows >= 2 and rows * W <= 64]
    assert sorted(got) == sorted(ENABLED)
    # and a grid the rule leaves out because the barrier would hand the saving back: 8 x 64 on the 512-row tile, only wave 0 / 7 hold an edge row
    per_wave = [bin(dead_mask(8, 64, wm, 0, 0)).count("1") for wm in range(8)]
    assert per_wave[0] > 0 and per_wave[1] == 0


def test_a_quarter_of_the_pairs_is_dead_on_the_2x16_grid():
    for gh, gw, wm in itertools.product(range(2), range(2), range(4)):
        assert bin(dead_mask(2, 16, wm, gh, gw)).count("1") == 4   # of 16 (tap, fragment) pairs
    # 4 x 16: one fragment in four lies on each edge -> an eighth; 2 x 32: a quarter
    assert {bin(dead_mask(4, 16, wm, 0, 1)).count("1") for wm in range(4)} == {2}
    assert {bin(dead_mask(2, 32, wm, 1, 0)).count("1") for wm in range(4)} == {4}


def _tile_conv(x, w, rows, W, transposed, phase, skip):
    """One 256-pixel tile of whole images in the kernel's k order (class, tap), float32, fragment by fragment.
    x: conv [nseg, 2 rows, 2 W, C] / transposed conv [nseg, rows, W, C]; w[kh][kw]: [C, N].  Returns [256, N] (transposed: one phase)."""
    nseg, C, N = x.shape[0], x.shape[3], w.shape[3]
    acc = np.zeros((256, N), np.float32)
    zero = np.zeros(C, np.float32)
    for gh, gw in ([(phase >> 1, phase & 1)] if transposed else itertools.product(range(2), range(2))):
        for tt in range(4):
            a, b = tt >> 1, tt & 1
            if transposed:
                kh, kw = (a if gh else 1 - a), (b if gw else 1 - b)
            else:
                kh, kw = 2 * a + gh, 2 * b + gw
            for wm, mi in itertools.product(range(4), range(4)):
                if skip and (dead_mask(rows, W, wm, gh, gw) >> (4 * tt + mi)) & 1:
                    continue
                frag = np.empty((16, C), np.float32)
                for frow in range(16):
                    ml = wm * 64 + mi * 16 + frow
                    seg, rem = divmod(ml, rows * W)
                    il, jl = divmod(rem, W)
                    if transposed:
                        ih, iw = il + a + gh - 1, jl + b + gw - 1
                    else:
                        ih, iw = 2 * il + kh - 1, 2 * jl + kw - 1
                    inside = 0 <= ih < x.shape[1] and 0 <= iw < x.shape[2]
                    assert inside == (not (edge_of(ml, rows, W) & kill_of(tt, gh, gw))), "the address-table rule IS the padding"
                    frag[frow] = x[seg, ih, iw] if inside else zero
                r0 = wm * 64 + mi * 16
                acc[r0:r0 + 16] += frag @ w[kh, kw]
    return acc


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("rows,W", ENABLED)
def test_conv_without_the_masked_pairs_has_the_same_bits(rows, W, transposed):
    rng = np.random.default_rng(rows * 100 + W + transposed)
    nseg, C, N = 256 // (rows * W), 8, 8
    x = rng.standard_normal((nseg, rows, W, C) if transposed else (nseg, 2 * rows, 2 * W, C)).astype(np.float32)
    w = rng.standard_normal((2, 2, C, N) if transposed else (4, 4, C, N)).astype(np.float32)
    for phase in (range(4) if transposed else [0]):
        full = _tile_conv(x, w, rows, W, transposed, phase, skip=False)
        cut = _tile_conv(x, w, rows, W, transposed, phase, skip=True)
        assert np.array_equal(full.view(np.uint32), cut.view(np.uint32))
        # ... and the model is the layer: against a direct sum over the padded input
        if transposed:
            xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
            gh, gw = phase >> 1, phase & 1
            want = sum(xp[:, a + gh:a + gh + rows, b + gw:b + gw + W].reshape(-1, C).astype(np.float64) @ w[a if gh else 1 - a, b if gw else 1 - b].astype(np.float64)
                       for a in range(2) for b in range(2))
        else:
            xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
            want = sum(xp[:, kh:kh + 2 * rows:2, kw:kw + 2 * W:2].reshape(-1, C).astype(np.float64) @ w[kh, kw].astype(np.float64)
                       for kh in range(4) for kw in range(4))
        assert np.allclose(full, want, rtol=1e-4, atol=1e-4)
