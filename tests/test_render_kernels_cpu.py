"""CPU: the table of tests/render_kernels.py reaches every cell of its coverage lists, every float32 restatement of a kernel's algorithm
stays under the ceiling of its (family, kind) -- an eighth of the tau the GPU test holds the kernel to -- against the float64 reference on
every row, every mutant of a restatement leaves the bound on the rows named for it by MIN_MARGIN at the least (test_zz_mutant_margins
prints the margins and the worst restatement ratios with -s), the composed restatement (spectra -> frames -> mix) is inside the chain's
bound, no element is left out of a comparison, and the restated launch geometry is the source's."""
import os

import numpy as np
import pytest

import feeder_kernels as Fk
import render_kernels as Rk
from elem_bound import TAU_FP32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNT = {"spectra": 36, "frames": 15, "mix": 15, "chain": 5}
MARGINS, WORST = {}, {}


def _ids(family, pred=lambda r: True):
    return [r["id"] for r in Rk.ROWS[family] if pred(r)]


@pytest.mark.parametrize("family", sorted(Rk.ROWS))
def test_rows_reach_every_cell(family):
    reached = {}
    for row in Rk.ROWS[family]:
        for c in Rk.cells(row):
            reached.setdefault(c, []).append(row["id"])
    missing = Rk.all_cells(family) - set(reached)
    assert not missing, sorted(map(str, missing))
    assert not set(reached) - Rk.all_cells(family), sorted(map(str, set(reached) - Rk.all_cells(family)))
    for c in sorted(Rk.all_cells(family), key=str):
        print("%-60s %s" % (c, ", ".join(reached[c][:3])))
    assert len({r["id"] for r in Rk.ROWS[family]}) == len(Rk.ROWS[family]) == ROW_COUNT[family]
    assert all(Rk.largest_buffer_bytes(r) <= 48 << 20 for r in Rk.ROWS[family])


def test_rows_are_windows_the_entry_points_admit():
    """m2h_render_frames' and m2h_render_mix's own window conditions, restated, hold on every row; the plan rows are render_plan's chunks."""
    from m2h.audio.render import render_plan
    for r in Rk.FRAMES_ROWS:
        _, j_lo, j_hi = Rk.frames_reads(r)
        assert 0 <= r["m0"] and r["m0"] + r["nm"] <= r["J"] + r["Pn"] - 1 and r["Pn"] <= Rk.RMAXP and r["K"] in (1, r["J"]), r["id"]
        assert 0 <= r["jx0"] <= j_lo and j_hi < r["jx0"] + r["nx"] <= r["J"], r["id"]
        assert (0 <= r["kh0"] <= j_lo and j_hi < r["kh0"] + r["nh"] <= r["J"]) if r["K"] != 1 else (r["kh0"] == 0 and r["nh"] == 1), r["id"]
    chunks = render_plan(2 * Rk.B + 1, Rk.B + 1, 1, 1, tail=True)["chunks"]
    plan = [r for r in Rk.FRAMES_ROWS if ".plan" in r["id"]]
    assert [(r["m0"], r["m0"] + r["nm"], r["jx0"], r["jx0"] + r["nx"]) for r in plan] == [c["frames"] + c["x"] for c in chunks] and len(plan) == 4
    for r in Rk.MIX_ROWS:
        f_lo, f_hi, n0, n1 = Rk.mix_window(r)
        assert 0 <= r["o0"] < r["o1"] and n0 < r["L_out"] and (r["o1"] - 1) * Rk.B < r["L_out"] and r["o1"] - 1 <= r["F"], r["id"]
        assert 0 <= r["m0"] <= f_lo and f_hi < r["m0"] + r["nm"], r["id"]
        mask = Rk.mix_read_mask(r)
        assert mask.any(1).tolist() == [f_lo <= r["m0"] + i <= f_hi for i in range(r["nm"])], r["id"]      # frames outside [f_lo, f_hi] are all NaN
        if r["o0"] >= 1:
            assert not mask[r["o0"] - 1 - r["m0"], :Rk.B].any()
        if r["o1"] - 1 < r["F"]:
            assert not mask[r["o1"] - 1 - r["m0"], Rk.B:].any()
    for r in Rk.SPECTRA_ROWS:
        assert (r["first_block"] + r["nblk"] - 1) * Rk.B < r["row_len"] and r["k0"] + r["n_mid"] <= r["K"], r["id"]


def test_restated_launch_geometry_is_the_sources():
    src = open(os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc", "render.hip")).read()
    assert "constexpr int RB = %d;" % Rk.B in src and "constexpr int RLOGM = %d;" % Rk.LOGM in src and "constexpr int RMAXP = %d;" % Rk.RMAXP in src
    assert "constexpr int RM = 1 << RLOGM;" in src and "constexpr int RFRAME = 2 * RB;" in src
    assert (Rk.B, Rk.M, Rk.RMAXP, Rk.PAIRS_PER_THREAD, Rk.GROUP, Rk.FRAME, Rk.NFFT) == (16000, 2 ** 14, 16, 8, 4, 32000, 32768)
    assert "constexpr int NP = %d;" % Rk.GROUP in src and "for (int grp = 0; grp < RM / 2 / %d / NP; ++grp) {" % Rk.TRANSFORM_BLOCK in src
    assert Rk.M // 2 // Rk.TRANSFORM_BLOCK // Rk.GROUP == 2                                      # 8 pairs per thread in two groups of 4
    assert "M2H_LAUNCH(render_spectra_kernel, dim3(nblk, n_mid * n_inner, n_outer), dim3(%d), sizeof(cf) << RLOGM" % Rk.TRANSFORM_BLOCK in src
    assert "M2H_LAUNCH(render_frames_kernel, dim3(nm, RS, 2), dim3(%d), sizeof(cf) << RLOGM" % Rk.TRANSFORM_BLOCK in src
    assert "const long long quads = ((long long)(o1 - o0) * RB) / 4;" in src
    assert "M2H_LAUNCH(render_mix_kernel, dim3((unsigned)((quads + %d) / %d), 2, R), dim3(%d), 0" % (Rk.MIX_BLOCK - 1, Rk.MIX_BLOCK, Rk.MIX_BLOCK) in src
    assert "const long long n = (long long)o0 * RB + 4ll * ((long long)blockIdx.x * %d + threadIdx.x);" % Rk.MIX_BLOCK in src
    row = Rk.ROWS_BY_ID["spectra.rir.Lr16001.K3.k1.mid2.noise"]
    assert Rk.spectra_grid(row) == ((2, 4, 2), 1024) and Rk.spectra_args(row) == (2 * 16001, (2, 2, 2, 3 * 16001 * 2, 16001 * 2, 1, 16001, 2, 0, 2))
    assert Rk.frames_grid(Rk.ROWS_BY_ID["frames.limit.RS1.J2.Pn16.K2.m0+17.x0+2.h0+2"]) == ((17, 1, 2), 1024)
    assert Rk.mix_grid(Rk.ROWS_BY_ID["mix.R2.S3.m0+3.F3.o0-3.L40001.images.custom"]) == ((47, 2, 2), 256)      # ceil(3 * 4000 / 256)
    assert Rk.mix_grid(Rk.ROWS_BY_ID["mix.R1.S1.m0+1.F1.o0-1.L1.images.default"]) == ((16, 2, 1), 256)
    assert Fk.MIN_MARGIN == Rk.MIN_MARGIN == 4.0


def test_every_mutant_has_rows_and_the_taus_are_the_stated_ones():
    for (f, m), pred in Rk.MUTANT_ROWS.items():
        assert sum(1 for r in Rk.ROWS[f] if pred(r)) >= 1, m
    every = {("spectra", m) for m in Rk.SPECTRA_MUTANTS} | {("frames", m) for m in Rk.FRAMES_MUTANTS} | {("mix", m) for m in Rk.MIX_MUTANTS}
    assert every == set(Rk.MUTANT_ROWS) and len(every) == 7 + 9 + 6
    assert all(Rk.TAU[k] == 8 * v for k, v in Rk.RESTATEMENT_WORST.items()) and Rk.TAU[("mix", "noise")] == TAU_FP32
    assert set(Rk.TAU) == {("spectra", k) for k in Rk.KINDS} | {("frames", "noise"), ("frames", "impulse"), ("mix", "noise"), ("chain", "noise"), ("chain", "dc")}


def test_slot_layout_round_trip():
    g = np.random.default_rng(1)
    S = g.standard_normal(Rk.M + 1) + 1j * g.standard_normal(Rk.M + 1)
    S[0], S[Rk.M] = S[0].real, S[Rk.M].real
    Z = Rk.to_slots(S)
    assert np.array_equal(Rk.from_slots(Z), S) and Z[0] == S[0].real + 1j * S[Rk.M].real
    assert Z[Rk.M // 2] == S[Rk.M // 2] and Z[Rk.M // 2 + 1] == np.conj(S[Rk.M // 2 + 1]) and Z[1] == S[1] and Z[Rk.M - 1] == np.conj(S[Rk.M - 1])
    x = g.standard_normal(Rk.NFFT)
    assert abs(Rk.energy(np.fft.rfft(x)) - (x * x).sum()) <= 1e-9 * (x * x).sum()


def _within(row, got, ref):
    worst_all = 0.0
    for name, (r, s) in ref.items():
        total = 0
        for kind, (worst, scale, ok, count) in Rk.compare(row, name, got[name], r, s).items():
            key = (row["family"], kind)
            assert ok and worst <= Rk.RESTATEMENT_WORST[key], ("restatement", row["id"], name, kind, worst, scale)
            WORST[key] = max(WORST.get(key, (0.0, "")), (worst, row["id"]))
            worst_all, total = max(worst_all, worst), total + count
        assert total == np.size(got[name]) == np.size(r), (row["id"], name)      # no element is left out
    return worst_all


def _margin(row, got, ref):
    """By how many tau the worst element of any output leaves its bound (inf: an exact or unwritten element differs, or a value is not finite)."""
    m = 0.0
    for name, (r, s) in ref.items():
        for kind, (worst, scale, ok, count) in Rk.compare(row, name, got[name], r, s).items():
            m = max(m, worst / Rk.tau_of(row["family"], kind) if worst == worst else float("inf"))
    return m


def _restatement_and_mutants(family, row):
    inp = Rk.inputs(row)
    ref = Rk.reference(row, inp)
    got = Rk.FP32[family](row, inp)
    worst = _within(row, got, ref)
    for (f, m), pred in Rk.MUTANT_ROWS.items():
        if f == family and pred(row):
            margin = _margin(row, Rk.FP32[family](row, inp, m), ref)
            MARGINS[(f, m)] = min(MARGINS.get((f, m), float("inf")), margin)
            assert margin >= Rk.MIN_MARGIN, (row["id"], m, margin)
    return inp, got, ref, worst


@pytest.mark.parametrize("row_id", _ids("spectra"))
def test_spectra_restatement_fits_and_mutants_do_not(row_id):
    row = Rk.ROWS_BY_ID[row_id]
    inp, got, ref, worst = _restatement_and_mutants("spectra", row)
    r, s = ref["spec"]
    assert np.isfinite(r).all() and not np.isnan(got["spec"]).any()
    assert np.isnan(inp["x"]).any() == (row["first_block"] > 0 or row["k0"] > 0)                 # what the window does not name is NaN
    if row["kind"] == "impulse":                                                                 # blocks before the impulse are exact zeros
        assert (s[..., :-1, :, :] == 0).all() and (got["spec"][..., :-1, :, :] == 0).all() and (s[..., -1, :, :] > 0).all()


@pytest.mark.parametrize("row_id", _ids("frames"))
def test_frames_restatement_fits_and_mutants_do_not(row_id):
    row = Rk.ROWS_BY_ID[row_id]
    inp, got, ref, worst = _restatement_and_mutants("frames", row)
    r, s = ref["frames"]
    assert np.isfinite(r).all() and (s > 0).all() and float(np.abs(r[..., Rk.FRAME - 1] / s[..., 0]).max()) < 1e-6      # sample 31999: the circular result's zero, but for the spectra's own float32 rounding
    fr, j_lo, j_hi = Rk.frames_reads(row)
    read_x = {j - row["jx0"] for _, ps in fr for _, j in ps}
    assert [bool(np.isnan(inp["xspec"][:, i]).all()) for i in range(row["nx"])] == [i not in read_x for i in range(row["nx"])]
    assert not np.isnan(inp["xspec"][:, sorted(read_x)]).any()
    if "slack" in row["id"] or ".plan" in row["id"]:
        assert np.isnan(inp["xspec"]).any() or np.isnan(inp["hspec"]).any() or row["nx"] == len(read_x)


@pytest.mark.parametrize("row_id", _ids("mix"))
def test_mix_restatement_fits_and_mutants_do_not(row_id):
    row = Rk.ROWS_BY_ID[row_id]
    inp, got, ref, worst = _restatement_and_mutants("mix", row)
    f_lo, f_hi, n0, n1 = Rk.mix_window(row)
    for name, (r, s) in ref.items():
        written = ~np.isnan(r)
        assert written[..., n0:n1].all() and not written[..., :n0].any() and not written[..., n1:].any()
    if row["images"]:
        assert np.array_equal(got["images"], ref["images"][0].astype(np.float32), equal_nan=True)


def test_chain_composed_restatement_is_inside_the_bound():
    """spectra -> frames -> mix in float32 against render_ref.render_f64: one restatement per case (the chunking does not change the arithmetic)."""
    seen = set()
    for row in Rk.CHAIN_ROWS:
        if Rk.chain_key(row) in seen:
            continue
        seen.add(Rk.chain_key(row))
        inp = Rk.inputs(row)
        worst = _within(row, Rk.chain_fp32(row, inp), Rk.reference(row, inp))
        print("%s  composed restatement %.2e" % (row["id"], worst))
    assert len(seen) == 3


def test_zz_mutant_margins():
    """(summary: by how many tau each mutant leaves the bound, the least over its named rows, and the worst restatement ratio per kind)"""
    for (family, m), v in sorted(MARGINS.items()):
        print("margin  %-8s %-46s %.1e" % (family, m, v))
    for (family, kind), (w, rid) in sorted(WORST.items()):
        print("worst restatement ratio  %-8s %-8s %.2e of ceiling %.2e (tau %.2e)  %s" % (family, kind, w, Rk.RESTATEMENT_WORST[(family, kind)], Rk.TAU[(family, kind)], rid))
    if len(MARGINS) == len(Rk.MUTANT_ROWS):      # (the whole file ran)
        assert min(MARGINS.values()) >= Rk.MIN_MARGIN
