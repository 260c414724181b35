"""CPU: the table of tests/separator_kernels.py reaches every cell of its coverage lists, every float32 restatement of a kernel's algorithm
stays inside half its family's tau against the float64 reference on every row, every mutant of a restatement leaves the bound on the rows
named for it by MIN_MARGIN at the least (test_zz_mutant_margins prints the margins and the worst restatement ratios with -s), no element is
left out of a comparison, and the restated launch geometry is the sources'."""
import os

import numpy as np
import pytest

import rollout_kernels
import separator_kernels as Sk
from elem_bound import TAU_FP32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNT = {"frames": 8, "post": 2, "pre": 3, "bin_rows": 4, "ola": 7, "xfade": 7, "resample": 21, "slice": 14}
MARGINS, WORST = {}, {}


def _ids(family, pred=lambda r: True):
    return [r["id"] for r in Sk.ROWS[family] if pred(r)]


@pytest.mark.parametrize("family", sorted(Sk.ROWS))
def test_rows_reach_every_cell(family):
    reached = {}
    for row in Sk.ROWS[family]:
        for c in Sk.cells(row):
            reached.setdefault(c, []).append(row["id"])
    missing = Sk.all_cells(family) - set(reached)
    assert not missing, sorted(map(str, missing))
    assert not set(reached) - Sk.all_cells(family), sorted(map(str, set(reached) - Sk.all_cells(family)))
    for c in sorted(Sk.all_cells(family), key=str):
        print("%-90s %s" % (c, ", ".join(reached[c][:3])))
    assert len({r["id"] for r in Sk.ROWS[family]}) == len(Sk.ROWS[family]) == ROW_COUNT[family]


def test_grid_stride_rows_enter_the_second_pass_at_the_smallest_launch():
    """frames at nseg R = 257, ola at nseg R = 1049, xfade at R = 1049 with hop 4000 and L = 16000: one batch row fewer fits one pass."""
    full = Sk.SEP_GRID_CAP * Sk.SEP_BLOCK
    f, o, x = Sk.ROWS_BY_ID["frames.R257.L15999.hop16000.s0.n1.big"], Sk.ROWS_BY_ID["ola.R1049.L16000.big"], Sk.ROWS_BY_ID["xfade.R1049.hop4000.L16000.big"]
    assert f["nseg"] * f["R"] == 257 and Sk.frames_total(f) > full >= Sk.frames_total(dict(f, R=256)) and Sk.second_pass(Sk.frames_total(f))
    assert o["R"] == 1049 and Sk.ola_total(o, o["calls"][0]) > full >= Sk.ola_total(dict(o, R=1048), o["calls"][0])
    assert x["R"] == 1049 and x["hop"] == 4000 and x["calls"] == ((0, 1, 0, 16000),)
    assert Sk.xf_total(x, x["calls"][0]) == 1049 * 4000 > full >= Sk.xf_total(dict(x, R=1048), x["calls"][0])
    assert not Sk.second_pass(full) and Sk.second_pass(full + 1) and Sk.sep_grid(0) == 1
    for fam in ("frames", "ola", "xfade"):
        assert [Sk.is_big(r) for r in Sk.ROWS[fam]].count(True) == 1
    # R in 1..3 and nseg in 1..3 everywhere else
    for r in Sk.FRAMES_ROWS:
        assert Sk.is_big(r) or (r["R"] <= 3 and r["nseg"] <= 3)
    for r in Sk.OLA_ROWS + Sk.XF_ROWS:
        assert Sk.is_big(r) or (r["R"] <= 3 and all(c[1] <= 3 for c in r["calls"])), r["id"]


def test_samples_one_and_two_frames_cover():
    """From sep_ola_sample's loop: one frame covers j = 0, the two samples 512 t - 1 and 512 t at every frame start t = 1 .. 31 (n = 1022 and
    1023 of the frame before lie past the 1022-point window) and, t1 being clamped, the 127 samples from 15873 on; two frames every other."""
    k = Sk.frames_per_sample()
    one = [0] + [512 * t + d for t in range(1, 32) for d in (-1, 0)] + list(range(15873, 16000))
    assert np.flatnonzero(k == 1).tolist() == one and set(k.tolist()) == {1, 2}


def test_resampler_choice_reaches_every_kernel():
    """rs_run's 8 -> 1 search, restated, over the ratios of tests/test_gpu_resample.py (RR.RATES, OTHER_KERNELS) and the two this table adds."""
    import resample_ref as RR
    from m2h.audio import resample as R
    seen = {}
    existing = list(RR.RATES) + [(128000, 16000), (256000, 16000), (512000, 16000), (32000, 3000), (1000, 1), (1023, 1000), (1000, 1023)]
    for f_in, f_out in existing + [(64000, 3000), (128000, 3000)]:
        seen.setdefault(Sk.rs_kernel(dict(f_in=f_in, f_out=f_out)), []).append((f_in, f_out))
    for k, ratio in Sk.RS_KERNEL_RATIOS.items():
        assert ratio in seen[k], (k, seen)
    # the existing ratios reach every kernel but the tiles of 512 and 256 outputs WITH a table: 64000 -> 3000 and 128000 -> 3000 are added for them
    old = {Sk.rs_kernel(dict(f_in=a, f_out=b)) for a, b in existing}
    assert set(Sk.RS_KERNEL_RATIOS) - old == {("tile 512", "table"), ("tile 256", "table")}
    assert Sk.rs_choice(1, 3, 61) == (2048, 4 * max(2048, Sk.rs_span_floats(2048, 1, 3, 61)))
    assert Sk.rs_choice(1, 1000, 20001) == (0, 0) and R.taps_per_output(1, 1000) == 20001
    for r in Sk.RS_ROWS:
        assert max(r["rows"] * r["cap"], r["rows"] * r["count"]) < 1 << 20, r["id"]


def test_restated_launch_geometry_is_the_sources():
    src = lambda n: open(os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc", n)).read()      # noqa: E731
    sep, rs, lay = src("separate.hip"), src("resample.hip"), src("layout.hip")
    assert "if (C == 2 && T % 2 == 0 && nblk <= 0x7fffffffL) {" in lay and "const long nblk = (long)B * (F / 16) * ((T + 63) / 64);" in lay
    assert "constexpr int TT = %d, LD = 132;" % Sk.SL_TT in lay and (Sk.SL_BLOCK, Sk.SL_GRID_CAP) == (256, 4096)
    assert "M2H_LAUNCH(sep_slice_input_kernel, dim3(grid_for(total, 256, 256 * 16)), dim3(256)" in lay
    assert "M2H_LAUNCH(sep_slice_input_plane_kernel, dim3(grid_for(total, 256, 256 * 16)), dim3(256)" in lay
    assert "const size_t total = (size_t)B * (F / 16) * T * (16 * C / 4);" in lay and "const size_t total = (size_t)B * (F / 16) * T * (ldo / 4);" in lay
    assert "size_t g = (total + block - 1) / block;" in lay and "if (g > cap) g = cap;" in lay
    assert "return m2h_sep_slice_input_fmt(mix, masks, out, B, F, T, C, 0, stream);" in lay
    assert "size_t g = (total + %d) / %d;" % (Sk.SEP_BLOCK - 1, Sk.SEP_BLOCK) in sep and "if (g > %d) g = %d;" % (Sk.SEP_GRID_CAP, Sk.SEP_GRID_CAP) in sep
    for name, v in (("SEP_SEG", Sk.SEP_SEG), ("SEP_T", Sk.SEP_T), ("SEP_NB", Sk.SEP_NB), ("SEP_LD", Sk.SEP_LD), ("SEP_NFFT", Sk.SEP_NFFT), ("SEP_NIFFT", Sk.SEP_NIFFT),
                    ("SEP_HOP", Sk.SEP_HOP), ("SEP_KT", Sk.SEP_KT)):
        assert "constexpr int %s = %d;" % (name, v) in sep, name
    assert "M2H_LAUNCH(sep_frames_kernel, dim3(sep_grid((size_t)nseg * R * 2 * SEP_T * (SEP_LD / 4))), dim3(%d)" % Sk.SEP_BLOCK in sep
    assert "M2H_LAUNCH(sep_istft_ola_kernel, dim3(sep_grid((size_t)nseg * R * (SEP_SEG / 4))), dim3(%d)" % Sk.SEP_BLOCK in sep
    assert "M2H_LAUNCH(sep_istft_xfade_kernel, dim3(sep_grid(quads * R)), dim3(%d)" % Sk.SEP_BLOCK in sep
    assert "const size_t quads = (size_t)((n_end - (long long)s0 * hop + 3) / 4);" in sep
    for k in ("sep_stft_post_kernel", "sep_istft_pre_kernel", "sep_bin_rows_kernel"):
        assert "M2H_LAUNCH(%s, dim3((unsigned)N * (SEP_NB / SEP_KT)), dim3(%d)" % (k, Sk.SEP_BLOCK) in sep
    assert "hop == SEP_SEG || hop == SEP_SEG / 2 || hop == SEP_SEG / 4" in sep and Sk.SEP_HOPS == (16000, 8000, 4000)
    assert "constexpr int RS_THREADS = %d;" % Sk.RS_THREADS in rs and "constexpr int RS_LDS_BYTES = %d * 1024;" % (Sk.RS_LDS_BYTES // 1024) in rs
    assert "constexpr int RS_MAX_RATIO = %d;" % Sk.RS_MAX_RATIO in rs
    assert "return up == 1 ? 0 : (long long)T * (up | 1);" in rs
    assert "const long long span = ((long long)(tile - 1) * down + up - 1) / up + T;" in rs and "return (span + 3 + 3) / 4 * 4;" in rs
    assert "for (int c = 8; c >= 1 && !npt; c >>= 1) {" in rs and "const int tile = RS_THREADS * c;" in rs and "if (f < tile) f = tile;" in rs
    assert "if (f * 4 <= RS_LDS_BYTES) {" in rs and "const int table_floats = (int)((table + 3) / 4 * 4);" in rs
    assert rollout_kernels.MIN_MARGIN == Sk.MIN_MARGIN == 4.0


def test_every_mutant_has_rows_and_the_taus_are_the_stated_ones():
    for (f, m), pred in Sk.MUTANT_ROWS.items():
        assert sum(1 for r in Sk.ROWS[f] if pred(r) and not Sk.is_big(r)) >= 1, m
    listed = Sk.FRAMES_MUTANTS + Sk.POST_MUTANTS + Sk.PRE_MUTANTS + Sk.BIN_MUTANTS + Sk.OLA_MUTANTS + Sk.XF_MUTANTS + Sk.RS_MUTANTS + Sk.SL_MUTANTS
    by_family = dict(frames=Sk.FRAMES_MUTANTS, post=Sk.POST_MUTANTS, pre=Sk.PRE_MUTANTS, bin_rows=Sk.BIN_MUTANTS, ola=Sk.OLA_MUTANTS, xfade=Sk.XF_MUTANTS,
                     resample=Sk.RS_MUTANTS, slice=Sk.SL_MUTANTS)
    every = {(f, m) for f, ms in by_family.items() for m in ms}
    assert every - set(Sk.MUTANT_ROWS) == {("xfade", "b unclamped")} and not set(Sk.MUTANT_ROWS) - every      # (dead code: test_xfade_b_clamp_is_dead)
    assert len(listed) == len(every) == 41
    assert all(Sk.TAU[f] == TAU_FP32 for f in Sk.FAMILIES)
    assert all(v <= TAU_FP32 / 2 for v in Sk.RESTATEMENT_WORST.values())
    long_chain = [r["id"] for rows in Sk.ROWS.values() for r in rows if Sk.tau_of(r) != TAU_FP32]
    assert long_chain == ["resample.1000-1.two_tiles+1.xoff0.yoff1"] and Sk.TAU_RS_LONG_CHAIN == 8 * Sk.RS_LONG_CHAIN_WORST == 1.4e-4


def _chk(got, rs, tau):
    """Sk.check of one output against its reference entry (r, s) or (r, s, where +inf is accepted)."""
    return Sk.check(got, rs[0], rs[1], tau, rs[2] if len(rs) > 2 else None)


def _within(family, row, got, ref):
    worst_all = 0.0
    for name, rs in ref.items():
        r, s = rs[0], rs[1]
        worst, scale, ok, count = _chk(got[name], rs, Sk.tau_of(row))
        assert count == np.size(got[name]) == np.size(r)                # no element is left out
        assert ok and worst <= Sk.restatement_limit(row), ("restatement", row["id"], name, worst, scale)
        worst_all = max(worst_all, worst)
    long_chain = Sk.tau_of(row) != Sk.TAU[family]
    key = family + " (long chain)" if long_chain else family
    WORST[key] = max(WORST.get(key, (0.0, "")), (worst_all, row["id"]))
    assert long_chain or worst_all <= Sk.RESTATEMENT_WORST[family], (row["id"], worst_all)
    return worst_all


def _margin(row, got, ref):
    m, tau = 0.0, Sk.tau_of(row)
    for name, rs in ref.items():
        worst = _chk(got[name], rs, tau)[0]
        m = max(m, worst / tau) if worst == worst else float("inf")
    return m


def _note(family, mutant, row, margin):
    MARGINS[(family, mutant)] = min(MARGINS.get((family, mutant), float("inf")), margin)
    assert margin >= Sk.MIN_MARGIN, (row["id"], mutant, margin)


def _restatement_and_mutants(family, row):
    inp = Sk.inputs(row)
    ref = Sk.reference(row, inp)
    got = Sk.FP32[family](row, inp)
    worst = _within(family, row, got, ref)
    for (f, m), pred in Sk.MUTANT_ROWS.items():
        if f == family and pred(row) and not Sk.is_big(row):
            _note(family, m, row, _margin(row, Sk.FP32[family](row, inp, m), ref))
    return inp, got, ref, worst


@pytest.mark.parametrize("row_id", _ids("frames"))
def test_frames_restatement_is_exact_and_mutants_are_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp, got, ref, worst = _restatement_and_mutants("frames", row)
    g = got["frames"]
    assert worst == 0.0 and not np.isnan(g).any() and float(np.abs(g[..., Sk.SEP_NFFT]).max()) == 0.0
    last = row["s0"] + row["nseg"] - 1
    if row["end"] - last * row["hop"] == 1:      # one sample: frame 0 holds it at n = 511 alone
        seg = g[-1]
        assert bool((seg[:, :, 0, 511] != 0).all()) and np.count_nonzero(seg) == np.count_nonzero(seg[:, :, 0, 511])


@pytest.mark.parametrize("row_id", _ids("post"))
def test_post_restatement_fits_and_mutants_do_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("post", row)
    r_ph, s_ph = ref["phasor"]
    zero = s_ph[..., 0] == 0
    assert zero.sum() >= 2 * Sk.SEP_NB and (r_ph[zero] == (1.0, 0.0)).all() and (got["phasor"][zero] == (1.0, 0.0)).all()
    r_mag, _, over = ref["mag"]
    assert np.isfinite(r_mag).all() and np.array_equal(np.isinf(got["mag"]), over) and over.sum() > 0 and np.isfinite(got["phasor"]).all()
    # +inf passes only where |X| is past the float32 range, a finite value inside the bound passes there too, nothing else does
    finite = np.where(over, r_mag, got["mag"]).astype(np.float32)
    assert _chk(finite, ref["mag"], Sk.TAU["post"])[2]
    assert not _chk(np.where(over, np.float32(80.0), got["mag"]), ref["mag"], Sk.TAU["post"])[2]
    k = np.flatnonzero(~over.reshape(-1))[0]
    spoiled = got["mag"].copy()
    spoiled.reshape(-1)[k] = np.inf
    assert not _chk(spoiled, ref["mag"], Sk.TAU["post"])[2]


@pytest.mark.parametrize("row_id", _ids("pre"))
def test_pre_restatement_fits_and_mutants_do_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("pre", row)
    off = (inp["P"][..., 0] <= 0).transpose(0, 2, 1).reshape(-1, Sk.SEP_NB)
    assert off.sum() > 1000 and (ref["rows"][0][:, :Sk.SEP_NB][off] == 0).all() and (got["rows"][:, Sk.SEP_NB:][off] == 0).all()


@pytest.mark.parametrize("row_id", _ids("bin_rows"))
def test_bin_rows_restatement_is_exact_and_mutants_are_not(row_id):
    assert _restatement_and_mutants("bin_rows", Sk.ROWS_BY_ID[row_id])[3] == 0.0


def _blocks(row):
    step = Sk.OLA_BLOCK if Sk.is_big(row) else row["R"]
    return [slice(i, min(i + step, row["R"])) for i in range(0, row["R"], step)]


@pytest.mark.parametrize("row_id", _ids("ola"))
def test_ola_restatement_fits_and_mutants_do_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    if not Sk.is_big(row):
        inp, got, ref, _ = _restatement_and_mutants("ola", row)
        r, s = ref["y"]
        past = np.arange(row["cap"]) + row["origin"] >= row["end"]
        assert np.isnan(r[:, past]).all() and np.isnan(got["y"][:, past]).all() and not np.isnan(r[:, ~past]).any()
        if row["wzero"]:
            assert (r[:, [0, 512]] == 0).all() and (s[:, [0, 512]] == 0).all() and (got["y"][:, [0, 512]] == 0).all() and bool((np.abs(r[:, 511]) < 1e-18).all())
        return
    inp = Sk.inputs(row)
    for rsel in _blocks(row):            # blocks of batch rows: host memory stays modest
        _within("ola", row, Sk.ola_fp32(row, inp, None, rsel), Sk.ola_reference(row, inp, rsel))


def _xfade_chain(row, inp, rsel=None, mutant=None, mutant_call=None):
    """Every call of the row on the float32 y the restatement's previous call left (LOCAL: the reference of a call starts from that y)."""
    R = row["R"]
    nr = len(range(*(rsel or slice(0, R)).indices(R)))
    y = np.full((nr, row["cap"]), np.nan, dtype=np.float32)
    for ci in range(len(row["calls"])):
        prior = Sk.xf_prior(row, ci, y)
        ref = Sk.xf_reference_call(row, inp, ci, prior, rsel)
        got = Sk.xf_fp32_call(row, inp, ci, prior, None, rsel)
        _within("xfade", row, got, ref)
        if mutant is not None:
            yield ci, prior, ref
        y = got["y"]


@pytest.mark.parametrize("row_id", _ids("xfade"))
def test_xfade_restatement_fits_and_mutants_do_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    if Sk.is_big(row):
        for rsel in _blocks(row):
            list(_xfade_chain(row, inp, rsel))
        return
    per_mutant = {}
    for ci, prior, ref in _xfade_chain(row, inp, mutant=True):
        for (f, m), pred in Sk.MUTANT_ROWS.items():
            if f == "xfade" and pred(row):      # a mutant must leave the bound on one call of the row at the least
                per_mutant[m] = max(per_mutant.get(m, 0.0), _margin(row, Sk.xf_fp32_call(row, inp, ci, prior, m), ref))
    for m, v in per_mutant.items():
        _note("xfade", m, row, v)
    # the last call leaves every sample below L written and nothing else
    L, origin = row["calls"][-1][3], row["calls"][-1][2]
    final = ref["y"][0]
    written = ~np.isnan(final[0])
    assert written[:L - origin].all() and not written[L - origin:].any()


@pytest.mark.parametrize("row_id", _ids("xfade", lambda r: not Sk.is_big(r)))
def test_xfade_b_clamp_is_dead(row_id):
    """b = n0 div hop never passes S - 1 for n0 < L: the mutant without the clamp is the restatement, bit for bit (margin 0, argued away in the
    module docstring of tests/separator_kernels.py)."""
    row = Sk.ROWS_BY_ID[row_id]
    inp = Sk.inputs(row)
    y = np.full((row["R"], row["cap"]), np.nan, dtype=np.float32)
    for ci, call in enumerate(row["calls"]):
        prior = Sk.xf_prior(row, ci, y)
        y = Sk.xf_fp32_call(row, inp, ci, prior)["y"]
        assert np.array_equal(y, Sk.xf_fp32_call(row, inp, ci, prior, "b unclamped")["y"], equal_nan=True)
        n = np.arange(*Sk.xf_span(row, call))
        a, b, S = Sk._xf_cover(row, call, n)
        assert int(b.max()) <= S - 1
    for L in range(1, 40000, 37):
        for hop in Sk.SEP_HOPS:
            assert (L - 1) // hop == -(-L // hop) - 1


@pytest.mark.parametrize("row_id", _ids("resample"))
def test_resample_restatement_fits_and_mutants_do_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp, got, ref, worst = _restatement_and_mutants("resample", row)
    print("%s  %s  restatement ratio %.2e" % (row_id, Sk.rs_kernel(row), worst))
    r = ref["y"][0]
    view = r[row["yoff"]:row["yoff"] + row["rows"] * row["count"]].reshape(row["rows"], row["count"])
    assert np.isnan(r[:row["yoff"]]).all() and np.isnan(r[row["yoff"] + view.size:]).all()
    if row["nan_rows"]:
        assert np.isnan(view[0::2]).all() and np.isfinite(view[1::2]).all()
    else:
        assert np.isfinite(view).all()


@pytest.mark.parametrize("row_id", _ids("slice"))
def test_slice_restatement_fits_and_mutants_do_not(row_id):
    row = Sk.ROWS_BY_ID[row_id]
    inp, got, ref, worst = _restatement_and_mutants("slice", row)
    r, s = ref["out"]
    if inp["masks"] is None and not row["split"]:
        assert worst == 0.0 and not s.any()
    if inp["masks"] is not None:      # exactly 0 where m (e - 1) <= 0
        off = Sk._sl_layout((inp["masks"] <= 0) | (inp["mix"] == 0))
        assert 0.3 < off.mean() < 0.7 and (r[off] == 0).all() and (got["out"][off] == 0).all() and (row["split"] or (s[off] == 0).all())
    if row["form"] == "plane":
        nc = 16 * row["C"]
        assert (r[..., nc] == inp["cls"][:, None, None]).all() and (r[..., nc + 1:] == 0).all() and r.shape[-1] == row["ldo"] > nc + 1


def test_slice_grid_stride_rows_are_the_smallest_launches_with_a_second_pass():
    full = Sk.SL_GRID_CAP * Sk.SL_BLOCK
    big = [r for r in Sk.SL_ROWS if Sk.is_big(r)]
    assert [Sk.sl_kernel(r) for r in big] == ["generic", "plane"] and all(Sk.sl_second_pass(r) for r in big)
    assert [Sk.sl_total(r) for r in big] == [full + 4, full + 4]      # a total is a multiple of 4 C or ldo / 4 and of Hs T: 4 x 262145 and 5 x 209716
    assert not any(Sk.sl_second_pass(r) for r in Sk.SL_ROWS if not Sk.is_big(r))
    # bfloat16 by ties-to-even: 1 + 2^-8 is a tie and goes down to 1, 1 + 3 x 2^-8 is a tie and goes up to 1 + 2^-6
    assert Sk.bf16_round(np.array([1.0, 1.00390625, 1.01171875, 1.0078125], dtype=np.float32)).tolist() == [1.0, 1.0, 1.015625, 1.0078125]
    v = np.array([3.14159274, -1e-3, 12.0], dtype=np.float32)
    packed = np.zeros(32, dtype=np.float32)
    hi = Sk.bf16_round(np.resize(v, 32))
    lo = Sk.bf16_round(np.resize(v, 32) - hi)
    packed.view(np.uint16)[:32], packed.view(np.uint16)[32:] = hi.view(np.uint32) >> 16, lo.view(np.uint32) >> 16
    assert np.array_equal(Sk.unsplit32(packed), hi.astype(np.float64) + lo) and float(np.abs(Sk.unsplit32(packed) / np.resize(v, 32) - 1).max()) <= 2.0 ** -17


def test_zz_mutant_margins():
    """(summary: by how many tau each mutant leaves the bound, the least over its named rows, and the worst restatement ratio per family)"""
    for (family, m), v in sorted(MARGINS.items()):
        print("margin  %-10s %-50s %.1e" % (family, m, v))
    for family, (w, rid) in sorted(WORST.items()):
        print("worst restatement ratio  %-10s %.2e  %s" % (family, w, rid))
    if len(MARGINS) == len(Sk.MUTANT_ROWS):      # (the whole file ran)
        assert min(MARGINS.values()) >= Sk.MIN_MARGIN
