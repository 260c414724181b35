"""CPU: the table of tests/strip_kernels.py reaches every cell of the strip kernels' launch arithmetic (csrc/conv_strip.hip), the restated job
map takes every job exactly once, the restated constants are the source's, CPU stand-ins of the kernels hold the element bound with a 3x
margin on every small row, every named mutant leaves it by MIN_MARGIN at the least on each row named for it, the float32 restatement of
the bin2mono pre-op stays under the ceiling TAU_PRE is 8 x of, and the HI rows' flag conditions hold.  Nothing here launches a kernel.
(-s prints the cells, the worst ratios and the margins.)

Measured here (python -m pytest tests/test_strip_kernels_cpu.py -s), ratios in units of the row's tau, held under 1 / 3:
  stand-ins, bf16x3 rows (TAU_BF16X3): fp32 conv 0.117 (first stage: the output's split32 rounding), 0.009 (last stage); hi*hi + hi*lo + lo*hi
    0.157 (c1.cls.b9.t256), 0.134 (masked, tiny_mask), 0.085 (last stage, both N)
  stand-ins, HI rows (TAU_FP32): 0.236 (first stage), 0.330 (masked), 0.322 / 0.317 (last stage N = 32 / 16)
  pre-op restatement |p32 - p64| / u: 2.59e-7 at the worst (tiny_mask; normal 1.9e-7 - 2.1e-7, loud 2.1e-7; the multi-round rows, measured once
    outside this file, 2.35e-7 and 2.12e-7) under the ceiling 2.8e-7; TAU_PRE = 2.24e-6
  HI rows: flagged 0.21 % of the pre-op's results (36.8 % of the outputs carry no allowance), 1.74 % / 1.76 % of Y (57.6 % / 75.7 %)
  mutants, smallest margin over the rows each is named for: left halo column as zeros 5.9 (quiet), halo records without lo 12, one group hi-only
    14, head reading Y's hi half 17, lo products left in (HI) 440, head bias twice 560, seam given the border's class 2.1e3, every other one
    above 4.9e3, the clamp dropped leaves NaN
  job map: 1600 small maps and 24 multi-round maps sound; both map mutants seen on every multi-round shape"""
import os
import re

import pytest
import torch

import strip_kernels as K
from elem_bound import TAU_BF16X3, TAU_FP32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS, WORST = {}, {}
_CACHE = {}


def _row_data(name):
    """(row, data, reference) of a small row, computed once and left unchanged."""
    if name not in _CACHE:
        row = K.ROWS[name]
        d = K.data(row)
        _CACHE[name] = (row, d, K.reference(row, d))
    return _CACHE[name]


def _note(m, margin, name):
    MARGINS[m] = min(MARGINS.get(m, (float("inf"), "")), (margin, name))
    print("mutant       %-28s %-56s %.1e" % (name, m, margin))
    assert margin >= K.MIN_MARGIN, (name, m, margin)


def _margin(g, ref):
    worst, scale, ok = K.check(g, ref)
    assert not ok
    return float("inf") if worst != worst else worst    # (NaN: the mutant left NaN behind)


def test_rows_reach_every_cell():
    for kernel, all_cells in K.ALL_CELLS.items():
        reached = {}
        for name, row in K.ROWS.items():
            if row["kernel"] != kernel or row["hi"]:
                continue
            shares = K.pre_ratio(row, _row_data(name)[1])[1] if row.get("masked") and not row["multi"] else None
            for c in K.cells(row, shares):
                reached.setdefault(c, []).append(name)
        for c in sorted(all_cells):
            print("%-8s %-28s %s" % (kernel, c, ", ".join(reached.get(c, [])[:4])))
        assert not all_cells - set(reached), sorted(all_cells - set(reached))
        assert not set(reached) - all_cells, sorted(set(reached) - all_cells)
    # the HI table: one small and one multi-round row per kernel
    assert sorted((r["kernel"], r["multi"]) for r in K.HI_ROWS) == sorted((k, m) for k in K.GRID_CAP for m in (False, True))


def test_rows_are_what_their_names_say():
    slots = {n: (K.jobs_padded(r["B"], K.strips_of(r)), K.GRID_CAP[r["kernel"]]) for n, r in K.ROWS.items() if r["multi"] and not r["hi"]}
    assert slots == {"c1.cls.b513.t64": (520, 512), "c1.msk.b513.t64": (520, 512), "c1.cls.b129.t256": (544, 512), "c1.msk.b129.t256": (544, 512),
                     "last32.b257.h2.w32": (264, 256), "last32.b65.h2.w128": (288, 256), "last16.b513.h2.w32": (520, 512), "last16.b260.h2.w64": (528, 512)}
    for n, r in K.ROWS.items():
        if r["multi"]:
            pick = K.compared_images(r)
            assert len(pick) == K.COMPARED_CAP == len(set(pick)) and all(0 <= b < r["B"] for b in pick), n
        else:
            assert K.jobs_padded(r["B"], K.strips_of(r)) <= 64 < min(K.GRID_CAP.values()), n     # one round
        if r["kernel"].startswith("conv1"):
            assert r["B"] * 512 * r["T"] * 2 * 4 < 136e6                                         # no input tensor above 135.3 MB (B = 129, T = 256)
    # reversed, B = 513 at one strip: workgroup 0 meets a live slot first, workgroups 1 .. 7 an empty one first and a live one second
    wgs = K.job_map(513, 1, 512, 1)[2]
    assert [j for _, j in wgs[0]] == [512, 0] and all([j for _, j in wgs[i]] == [-1, i] for i in range(1, 8)) and all(len(w) == 1 for w in wgs[8:])
    wgs = K.job_map(513, 1, 512, 0)[2]
    assert [j for _, j in wgs[0]] == [0, 512] and all([j for _, j in wgs[i]] == [i, -1] for i in range(1, 8))
    d = K.data(K.ROWS["c1.msk.wide.b2.t128"])
    assert float(d["scale"].min()) == pytest.approx(0.05) and float(d["scale"].max()) == pytest.approx(2.0)
    d = _row_data("c1.msk.b2.t128")[1]
    assert 0.30 < float((d["masks"] < 0).float().mean()) < 0.37                                     # a third of the masks clamp
    x = torch.arange(2 * 512 * 64 * 2, dtype=torch.float32).reshape(2, 512, 64, 2)
    y = K.slice_freq(x)
    for b, c, s, h, w in ((0, 0, 0, 0, 0), (1, 1, 15, 31, 63), (1, 0, 7, 5, 9), (0, 1, 3, 30, 2)):
        assert y[b, c * 16 + s, h, w] == x[b, s * 32 + h, w, c]


def test_job_map_sweep():
    """Every job exactly once, no slot outside [0, jobs_padded): B in 1 .. 40, strips 1 .. 4, both directions, both grid caps -- and, so that
    the restatement's own second round is under the sweep too, caps of 8, 16 and 24 workgroups; then the table's multi-round shapes."""
    n = 0
    for B in range(1, 41):
        for strips in (1, 2, 3, 4):
            for rev in (0, 1):
                for cap in (256, 512, 8, 16, 24):
                    assert K.map_faults(B, strips, cap, rev) == [], (B, strips, rev, cap)
                    n += 1
    multi = [r for r in K.ROWS.values() if r["multi"]]
    for r in multi:
        for rev in (0, 1):
            assert K.map_faults(r["B"], K.strips_of(r), K.GRID_CAP[r["kernel"]], rev) == []
    # the two mutants of the map are seen on every multi-round shape (M_REV_OFF in the reversed direction, the only one it touches)
    for r in multi:
        args = (r["B"], K.strips_of(r), K.GRID_CAP[r["kernel"]])
        assert K.map_faults(*args, 0, K.M_ROUND) and K.map_faults(*args, 1, K.M_ROUND) and K.map_faults(*args, 1, K.M_REV_OFF), r["id"]
        assert K.map_faults(*args, 0, K.M_REV_OFF) == []
    print("job map: %d small maps and %d multi-round maps sound; both mutants seen on every multi-round shape" % (n, 2 * len(multi)))


def test_constants_are_the_sources():
    src = open(os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc", "conv_strip.hip")).read()
    hdr = open(os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc", "m2h_internal.h")).read()

    def const(name):
        m = re.search(r"constexpr int %s = ([^;,]+)[;,]" % name, src)
        assert m, name
        return m.group(1).strip()

    assert int(const("SW")) == K.SW and const("PX") == "SW + 2" and K.PX == K.SW + 2
    assert const("RING") == str(K.RING["last"]) and "__shared__ __attribute__((aligned(1024))) char s_ring[%d * ROW];" % K.RING["conv1"] in src
    for text in ("const int grid = p.jobs_padded < %d ? p.jobs_padded : %d;" % (K.GRID_CAP["conv1"], K.GRID_CAP["conv1"]),
                 "convT_last_strip_kernel<32>), dim3(p.jobs_padded < %d ? p.jobs_padded : %d), dim3(512)" % (K.GRID_CAP["last32"], K.GRID_CAP["last32"]),
                 "convT_last_strip_kernel<16>), dim3(p.jobs_padded < %d ? p.jobs_padded : %d), dim3(256)" % (K.GRID_CAP["last16"], K.GRID_CAP["last16"]),
                 "convT_last_strip_kernel<32, true>), dim3(p.jobs_padded < %d ?" % K.GRID_CAP["last32"],
                 "convT_last_strip_kernel<16, true>), dim3(p.jobs_padded < %d ?" % K.GRID_CAP["last16"],
                 "p.jobs_padded = (B + 7) / 8 * 8 * p.strips;",
                 "const int xcd = linear & 7, y = linear >> 3;", "const int img = (y / strips) * 8 + xcd;", "const int job = img * strips + (y % strips);",
                 "return job < jobs ? job : -1;",
                 "strip_job(p.rev ? p.jobs_padded - 8 - (lin & ~7) + (lin & 7) : lin, p.strips, p.jobs);",
                 "for (int lin = blockIdx.x; lin < p.jobs_padded; lin += gridDim.x) {",
                 "p.rev = masks != nullptr ? (g_strip_rev & 1) : ((g_strip_rev >> 2) & 1);", "p.rev = ((g_strip_rev >> 1) & 1) ^ 1;",
                 "const bool has_l = r0 > 0, has_r = r0 + SW < p.Wq;",
                 "const int cw0 = (m == 0 && !has_l) ? 0 : 1, cw1 = (m == 15 && !has_r) ? 2 : 1;", "const int ch = q == 0 ? 0 : (q == 15 ? 2 : 1);",
                 "const bool okr = (unsigned)hi_ < 32u;", "const bool okr = (unsigned)h < (unsigned)p.Hq;"):
        assert text in src, text
    assert src.count("strip_job(p.rev ?") == 2 and "#define g_strip_rev (::m2h::tl_tuning.v[%d])" % K.REV_KNOB in hdr
    for text in ("const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f);", "const float z = fmaxf(m * (e - 1.f), 0.f);", "const float u = 1.f + z;",
                 "const float d = u - 1.f;", "(__builtin_amdgcn_logf(u) * 0.693147180559945309f) * (z * __builtin_amdgcn_rcpf(d));", "return d == 0.f ? z : r;"):
        assert text in hdr, text
    for k, label in K.LABEL.items():
        assert '"%s"' % label in src, label
    assert K.MIN_MARGIN == 4.0 and K.TAU_PRE == 8 * K.PRE_RESTATEMENT_WORST and K.PRE_RESTATEMENT_WORST == 2.8e-7
    assert (K.FLAG_SHARE_MAX, K.CLEAN_SHARE_MIN, K.COMPARED_CAP, K.OUT_ROUNDING) == (0.05, 0.25, 48, 2.0 ** -17)
    assert all(v and set(v) <= set(K.SMALL_ROWS) for v in K.MUTANT_ROWS.values()), [m for m, v in K.MUTANT_ROWS.items() if not v]


@pytest.mark.parametrize("name", [n for n in K.SMALL_ROWS if K.ROWS[n].get("masked")])
def test_pre_op_restatement_stays_under_its_ceiling(name):
    row, d, _ = _row_data(name)
    worst, shares = K.pre_ratio(row, d)
    print("pre-op       %-28s |p32 - p64| / u %.3e of ceiling %.3e (TAU_PRE %.3e)   %s" % (name, worst, K.PRE_RESTATEMENT_WORST, K.TAU_PRE,
                                                                                         "  ".join("%s %.3f" % kv for kv in shares.items())))
    WORST["pre-op"] = max(WORST.get("pre-op", (0.0, "")), (worst, name))
    assert worst <= K.PRE_RESTATEMENT_WORST, (name, worst)


@pytest.mark.parametrize("name", [n for n in K.SMALL_ROWS if not K.ROWS[n]["hi"]])
def test_stand_ins_hold_the_bound_and_mutants_do_not(name):
    row, d, ref = _row_data(name)
    assert ref["tau"] == TAU_BF16X3
    for kind in ("fp32", "x3"):
        worst, scale, ok = K.check(K.stand_in(row, d, kind), ref, margin=3.0)
        print("stand-in     %-28s %-5s worst %.3f tau  scale-1 %+.1e" % (name, kind, worst, scale - 1.0))
        WORST[(row["kernel"], kind)] = max(WORST.get((row["kernel"], kind), (0.0, "")), (worst, name))
        assert ok, (name, kind, worst, scale)
    for m, names in K.MUTANT_ROWS.items():
        if name in names:
            g = K.stand_in(row, d, "x3", m) if m == K.M_D0 else K.reference(row, d, m)["r"]
            _note(m, _margin(g, ref), name)


@pytest.mark.parametrize("name", [n for n in K.SMALL_ROWS if K.ROWS[n]["hi"]])
def test_hi_rows_flag_little_and_reject_the_bf16x3_result(name):
    row, d, ref = _row_data(name)
    assert ref["tau"] == TAU_FP32
    if "flagged" in ref:     # the two conditions that keep the allowance from hiding a failure, from the reference alone
        print("HI           %-28s flagged %.4f of the intermediate, %.3f of the outputs carry no allowance" % (name, ref["flagged"], ref["clean"]))
        assert ref["flagged"] <= K.FLAG_SHARE_MAX and ref["clean"] >= K.CLEAN_SHARE_MIN, (name, ref["flagged"], ref["clean"])
    else:
        assert row["kernel"] == "conv1" and float(ref["extra"].min()) >= 0 and ref["clean"] == 1.0
    worst, scale, ok = K.check(K.hi_stand_in(row, d), ref, margin=3.0)
    print("stand-in     %-28s fp32  worst %.3f tau  scale-1 %+.1e" % (name, worst, scale - 1.0))
    WORST[(row["kernel"], "hi")] = max(WORST.get((row["kernel"], "hi"), (0.0, "")), (worst, name))
    assert ok, (name, worst, scale)
    _note(K.M_LO_IN, _margin(K.reference(dict(row, hi=False), d)["r"], ref), name)


def test_zz_margins_and_worst_ratios():
    for m, (v, name) in sorted(MARGINS.items()):
        print("margin  %-56s %.1e  %s" % (m, v, name))
    for k, (w, name) in sorted(WORST.items(), key=str):
        print("worst   %-20s %.3e  %s" % (k, w, name))
    if len(MARGINS) == len(K.MUTANT_ROWS):      # (the whole file ran)
        assert min(v for v, _ in MARGINS.values()) >= K.MIN_MARGIN
