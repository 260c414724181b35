"""CPU: the tables of tests/row3x3_kernels.py reach every cell of the image-row 3x3 kernels' paths (csrc/wgrad_row3x3.hip,
csrc/conv_row3x3.hip), the restated launch arithmetic is the source's (and, for the split count, the library's own size function's), float32
stand-ins of the kernels hold the element bound with a 3x margin on every row, every named mutant leaves it by MIN_MARGIN at the least on
each row named for it, and the L1 rows' flagged shares stay under their caps.  Nothing here launches a kernel.  (-s prints the cells, the
worst ratios and the margins.)

Measured here (python -m pytest tests/test_row3x3_kernels_cpu.py -s), ratios in units of the row's tau, held under 1 / 3:
  stand-ins, weight gradient: fp32 sums 0.112 (fp32<16>), 0.100 (fp32<32>), 0.011 on the bf16x3 rows; three split products 0.111 (x3<16>), 0.108 (x3<32>);
    fused 0.0008 (fp32) / 0.031 (three products in both sums; wg.fused.n32.b1h1: its bound is loose, row3x3_kernels.py's docstring)
  stand-ins, forward: fp32 0.100 - 0.130 per instantiation, three products 0.115 - 0.132; input gradient: fp32 0.095 - 0.173 (fp32<32,16>,
    b513h4), three products 0.112 - 0.128; the two rows that are not the engine's 0.126
  L1: flagged share 7.6e-6 / 7.5e-6 / 8.8e-6 (fp32, B = 64 / 65 / 97; cap 5e-5), 5.3e-5 / 6.5e-5 / 6.0e-5 (bf16x3; cap 5e-4); the stand-ins' loss
    0.0025 (fp32) and 0.0006 (three products) tau, no unflagged gradient element wrong
  mutants, smallest margin over the rows each is named for (tau): fused w2 hi only 7.5 (the single-row row, the one it is named for), lo * hi term
    dropped 23, fused ring row from the next image 52, fused inner gradient ungated 410, fused inner taps not mirrored 680, L1 partials beyond
    block 511 dropped 1.0e3, bias after the activation 1.4e3, previous image's row 2.7e3, wrap at pixel column -1 / 32 2.8e3, slope ignored 2.9e3,
    split's first row dropped 3.8e3, stale validity mask 9.6e3, gate >= 0 1.2e4, gate at stride N 1.4e4, neighbouring image's halo row 1.6e4,
    column shift mirrored 2.1e4, mirrored taps walked forward 3.2e4, de-slice band and row swapped 3.7e4; L1 wrong count and reversed sign leave
    the exact gradient (infinite margin)
  the fused rows' second scale s_rms: stand-ins 0.005 (fp32) / 0.069 (three products; wg.fused.n32.b3h32); on EVERY fused row w2 hi only leaves tau by
    15 - 19 and the outer sum's dropped lo * hi term by 14 - 18
  109 tests, 21 s
"""
import os

import pytest

import row3x3_kernels as K
import wgrad_routes as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc")
MARGINS, WORST = {}, {}


def _note(m, margin, name):
    MARGINS[m] = min(MARGINS.get(m, (float("inf"), "")), (margin, name))
    print("mutant       %-44s %-72s %.1e" % (name, m, margin))
    assert margin >= K.MIN_MARGIN, (name, m, margin)


def _margin(g, ref):
    worst, scale, ok = K.check(g, ref)
    assert not ok
    return float("inf") if worst != worst else worst


def _stand_ins(name, kernel, math, fn, ref):
    for kind in ("fp32",) + (("x3",) if math == "x3" else ()):
        worst, scale, ok = K.check(fn(kind), ref, margin=3.0)
        print("stand-in     %-44s %-5s worst %.3f tau  scale-1 %+.1e" % (name, kind, worst, scale - 1.0))
        WORST[(kernel, kind)] = max(WORST.get((kernel, kind), (0.0, "")), (worst, name))
        assert ok, (name, kind, worst, scale)


def test_rows_reach_every_cell():
    for rows, cells_of, all_cells in ((K.WG_ROWS, K.wg_cells, K.wg_all_cells()), (K.FW_ROWS_TABLE, K.fw_cells, K.fw_all_cells())):
        reached = {}
        for name, row in rows.items():
            for c in cells_of(row):
                reached.setdefault(c, []).append(name)
        for c in sorted(all_cells, key=str):
            print("%-60s %s" % (" / ".join(c), ", ".join(reached.get(c, [])[:3])))
        assert not all_cells - set(reached), sorted(all_cells - set(reached), key=str)
    # the H = 1, 2, 3 rows and the forced S = 1 rows exist for all five weight-gradient kernels; no row above 3 x 32 image rows
    for k in K.WG_KERNELS:
        mine = [r for r in K.WG_ROWS.values() if K.wg_kernel(r) == k]
        assert {1, 2, 3} <= {r["H"] for r in mine} and any(r["knob11"] == 1 and r["B"] > 1 for r in mine), k
    assert max(r["B"] * r["H"] for r in K.WG_ROWS.values()) == 96
    assert all(K.wg_rule(r["N"], r["ldy"]) and r["ldy"] >= r["N"] for r in K.WG_ROWS.values())
    # forward: no input above 20 MB; every row is the engine's, the two `other` rows are not
    for r in K.FW_ROWS_TABLE.values():
        assert r["B"] * r["H"] * 32 * r["C0"] * 4 <= 20e6, r["id"]
        assert K.fw_kernel(r["math"], r["N"], r["C0"], r["B"], r["H"], r["deslice"]) is not None, r["id"]
    assert all(K.fw_kernel("x3", r["N"], r["C0"], r["B"], r["H"]) is None and K.fw_kernel("fp32", r["N"], r["C0"], r["B"], r["H"]) for r in K.OTHER_ROWS.values())
    assert len(K.MUTANT_ROWS) == 20 and all(v for v in K.MUTANT_ROWS.values()), [m for m, v in K.MUTANT_ROWS.items() if not v]


def test_rows_are_what_their_names_say():
    S = {(B, H, k): K.wg_S(B, H, k) for B, H, k in K.WG_SHAPES}
    assert S == {(1, 1, 0): 1, (5, 1, 0): 1, (3, 2, 0): 1, (5, 2, 0): 2, (6, 3, 0): 4, (17, 4, 0): 17, (13, 5, 0): 16, (3, 7, 0): 5, (3, 7, 1): 1, (3, 7, 2): 2,
                 (5, 8, 0): 10, (3, 32, 0): 24}
    assert K.wg_splits(6, 3, 4) == [(0, 4), (4, 9), (9, 13), (13, 18)] and K.wg_splits(3, 7, 5) == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 21)]
    # image starts on every phase of row & 3 (B 3, H 7 and B 13, H 5) and of row % 5 (B 3, H 7 and B 6, H 3)
    assert {(b * 7) & 3 for b in range(3)} | {(b * 5) & 3 for b in range(13)} == {0, 1, 2, 3} and {(b * 7) % 5 for b in range(3)} | {(b * 3) % 5 for b in range(6)} == {0, 1, 2, 3, 4}
    rounds = {n: (K.fw_chunks(r["B"], r["H"]), K.fw_grid(r["math"], r["N"], r["C0"], r["B"], r["H"]), K.fw_rounds(r)) for n, r in K.FW_ROWS_TABLE.items()}
    assert rounds["fwd.fp32.n32c32.b513h4.bias"] == (513, 512, 2) and rounds["fwd.x3.n32c32.b513h4.leaky"] == (513, 512, 2)
    assert rounds["dgrad.x3.n32c16.b769h4"] == (769, 768, 2) and rounds["fwd.x3.n16c32.b769h4.deslice"] == (769, 768, 2)
    assert rounds["fwd.fp32.n16c32.b1100h4.leaky"] == (1100, 512, 3) and rounds["fwd.x3.n16c32.b512h4.deslice"] == (512, 512, 1)
    assert rounds["fwd.fp32.n32c32.b65h32.deslice"] == (520, 512, 2) and rounds["fwd.x3.n32c16.b65h32.bias"] == (520, 520, 1)
    # at H = 4, 8, 32 the grid is a whole number of images: a later chunk has its predecessor's place in the image; at H = 20 it has not
    assert all(bool(K.fw_stale_chunks(r)) == (r["H"] == 20) for r in K.FW_ROWS_TABLE.values())
    assert K.fw_stale_chunks(K.FW_ROWS_TABLE["fwd.fp32.n32c32.b103h20"]) == [(512, 0), (514, 2)]
    assert K.fw_halo(512, 20) == (102, 8, True, True) and K.fw_halo(0, 20) == (0, 0, False, True) and K.fw_halo(514, 20) == (102, 16, True, False)
    # L1: B = 64 one chunk per block; B = 65: 520 chunks, eight fp32 blocks take a second one (none in bf16x3); B = 97: 776 chunks on 768 / 512 blocks
    two = lambda m, B: sum(len(w) > 1 for w in K.fw_walk(m, 16, 32, B, 32))   # noqa: E731
    assert [two(m, B) for m in ("fp32", "x3") for B in (64, 65, 97)] == [0, 8, 264, 0, 0, 8]


def test_launch_arithmetic_is_the_sources():
    wg = open(os.path.join(CSRC, "wgrad_row3x3.hip")).read()
    bwd = open(os.path.join(CSRC, "conv_bwd.hip")).read()
    fw = open(os.path.join(CSRC, "conv_row3x3.hip")).read()
    hdr = open(os.path.join(CSRC, "m2h_internal.h")).read()
    for text in ("const long target = g_wgrad_blocks > 0 ? g_wgrad_blocks : (wgrad_row3x3_rule(p, false) ? %d : 512);" % K.WG_TARGET,
                 "if (S > p.chunks / %d) S = p.chunks / %d;" % (K.WG_MIN_CHUNKS, K.WG_MIN_CHUNKS), "if (S > %d) S = %d;" % (K.WG_SMAX, K.WG_SMAX), "if (S < 1) S = 1;",
                 "int rc = launch_wgrad_row3x3(p, st);", "if (rc == NOT_THIS_ENGINE) rc = launch_wgrad_tiled(p, st);"):
        assert text in bwd, text
    for text in ("p.chunks = p.B * p.Hq;   // one image row per reduction chunk", "if (p.S > p.chunks) p.S = p.chunks;", "const dim3 grid((unsigned)p.S), blk(256);",
                 "p.C0 == 32 && p.C1 == 0 && p.Wq == 32 && p.Wi == 32 && p.Hq == p.Hi && p.direct && p.N <= 32 && p.N % 4 == 0;",
                 "return shape && (!launch || (p.ldy % 4 == 0 && g_wgrad_row3x3 >= 0 && p.ntiles * p.ktiles == 1));",
                 "if (p.dy2 != nullptr) M2H_LAUNCH(wgrad3x3_row_dgrad_bf16x3_kernel, grid, blk, 0, st, p);", "else if (tl_math_mode == 1) {",
                 "if (p.N <= 16) M2H_LAUNCH((wgrad3x3_row_bf16x3_kernel<16>), grid, blk, 0, st, p);", "else M2H_LAUNCH((wgrad3x3_row_bf16x3_kernel<32>), grid, blk, 0, st, p);",
                 "} else if (p.N <= 16) M2H_LAUNCH((wgrad3x3_row_kernel<16>), grid, blk, 0, st, p);", "else M2H_LAUNCH((wgrad3x3_row_kernel<32>), grid, blk, 0, st, p);",
                 "XT[4][C * WRB_RS];      // ring over image rows (slot = row & 3)", "auto slot5 = [](int r) { return (r + 5) % 5; };",
                 "const int t_lo = FR == 32 ? 0 : ((wave >> 1) ? 5 : 0), t_hi = FR == 32 ? 9 : ((wave >> 1) ? 9 : 5);"):
        assert text in wg, text
    assert wg.count("const int c0 = (int)(((long)p.chunks * split) / p.S), c1 = (int)(((long)p.chunks * (split + 1)) / p.S);") == 3
    for text in ("constexpr int W = 32, PW = W + 2, ROWS = %d, PR = ROWS + 2;" % K.FW_ROWS, "(long)p.B * (p.Hq / 4) >= %d &&" % K.FW_MIN_CHUNKS,
                 "p.Hq % 4 == 0 && p.N <= 32 && p.N % 4 == 0 && p.scale == nullptr", "(p.out_mode == M2H_OUT_NHWC || p.N % 16 == 0);",
                 "const long chunks = (long)p.B * (p.Hq / 4);", "if (p.math == 0 && (p.C0 == 16 || p.C0 == 32)) {",
                 "grid = dim3((unsigned)(chunks < %d ? chunks : %d));" % (K.FW_CAP, K.FW_CAP),
                 "} else if (p.math == 1 && (p.C0 == 32 || (p.C0 == 16 && p.N > 16))) {",
                 "const long cap = (p.N > 16 && p.C0 == 32) ? %d : %d;" % (K.FW_CAP, K.FW_CAP_NARROW), "grid = dim3((unsigned)(chunks < cap ? chunks : cap));",
                 "if (p.N <= 16 && p.C0 == 32) M2H_LAUNCH((conv3x3_row_kernel<16, 32>), grid, blk, 0, st, p);",
                 "else if (p.N <= 16) M2H_LAUNCH((conv3x3_row_kernel<16, 16>), grid, blk, 0, st, p);",
                 "else if (p.C0 == 32) M2H_LAUNCH((conv3x3_row_kernel<32, 32>), grid, blk, 0, st, p);", "else M2H_LAUNCH((conv3x3_row_kernel<32, 16>), grid, blk, 0, st, p);",
                 "if (p.N <= 16) M2H_LAUNCH((conv3x3_row_bf16x3_kernel<16, 32>), grid, blk, 0, st, p);",
                 "else if (p.C0 == 32) M2H_LAUNCH((conv3x3_row_bf16x3_kernel<32, 32>), grid, blk, 0, st, p);",
                 "else M2H_LAUNCH((conv3x3_row_bf16x3_kernel<32, 16>), grid, blk, 0, st, p);",
                 "ConvL1 l1 = {gt_plane, partials, loss, 1.f / ((float)B * 16.f * (float)H * (float)T)};",
                 "M2H_LAUNCH(l1_partials_sum_kernel, dim3(1), dim3(256), 0, st, p.l1_part, (int)grid.x, p.l1_inv, l1_loss);"):
        assert text in fw, text
    assert fw.count("for (int c = blockIdx.x; c < chunks; c += gridDim.x) {") == 2 and fw.count("const int b = c / (p.Hq / ROWS), q0 = (c - b * (p.Hq / ROWS)) * ROWS;") == 2
    assert fw.count("const bool ok = i < PR * PW * SEG && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)W;") == 2
    for label in list(K.FW_LABEL.values()) + list(K.L1_LABEL.values()):
        assert '"%s"' % label in fw, label
    red = open(os.path.join(CSRC, "wgrad_reduce.hip")).read()
    assert all('launch_status("%s")' % v in red for v in K.WG_LABEL.values())
    for knob, name in ((K.KNOB_BLOCKS, "g_wgrad_blocks"), (K.KNOB_WG_ROW, "g_wgrad_row3x3"), (K.KNOB_FW_ROW, "g_row3x3")):
        assert "#define %s (::m2h::tl_tuning.v[%d])" % (name, knob) in hdr
    # the split count against the library's own size function (host code): S = workspace / (N x 384 floats)
    for r in K.WG_ROWS.values():
        row = dict(B=r["B"], H=r["H"], W=32, C0=32, C1=0, N=r["N"], k=3, s=1, p=1, entry="packed", knobs={K.KNOB_BLOCKS: r["knob11"]} if r["knob11"] else {})
        assert WR.workspace_bytes(row) == K.wg_S(r["B"], r["H"], r["knob11"]) * r["N"] * K.KPAD * 4, r["id"]
    assert K.MIN_MARGIN == 4.0 and K.FLAG_CAP == {"fp32": 5e-5, "x3": 5e-4}


@pytest.mark.parametrize("name", list(K.WG_ROWS))
def test_weight_gradient_stand_ins_hold_the_bound_and_mutants_do_not(name):
    row = K.WG_ROWS[name]
    d = K.wg_data(row)
    ref = K.wg_reference(row, d)
    if row["gate"] is not None:
        assert 0.45 < float((d["gate"] == 0).float().mean()) < 0.55
    _stand_ins(name, K.wg_kernel(row), row["math"], lambda kind: K.wg_stand_in(row, d, kind), ref)
    for m, names in K.MUTANT_ROWS.items():
        if name in names:
            _note(m, _margin(K.wg_reference(row, d, m)["r"], ref), name)
    if row["fused"]:       # the second, tighter scale: the stand-ins hold it with the same 3x margin, a 2^-9 error of either sum's operands does not
        _stand_ins(name, "fused (s_rms)", "x3", lambda kind: K.wg_stand_in(row, d, kind), K.rms(ref))
        for m, names in K.MUTANT_ROWS_RMS.items():
            assert name in names
            _note(m + " (s_rms)", _margin(K.wg_reference(row, d, m)["r"], K.rms(ref)), name)


@pytest.mark.parametrize("name", list(K.FW_ROWS_TABLE) + list(K.OTHER_ROWS))
def test_forward_stand_ins_hold_the_bound_and_mutants_do_not(name):
    row = K.FW_ROWS_TABLE.get(name) or K.OTHER_ROWS[name]
    d = K.fw_data(row)
    ref = K.fw_reference(row, d)
    _stand_ins(name, "%s %s" % (row["dir"], K.fw_kernel(row["math"], row["N"], row["C0"], row["B"], row["H"], row["deslice"])), row["math"],
               lambda kind: K.fw_stand_in(row, d, kind), ref)
    for m, names in K.MUTANT_ROWS.items():
        if name in names:
            _note(m, _margin(K.fw_reference(row, d, m)["r"], ref), name)


@pytest.mark.parametrize("name", list(K.L1_ROWS))
def test_l1_flagged_share_stand_ins_and_mutants(name):
    row = K.L1_ROWS[name]
    d = K.l1_data(row)
    ref = K.l1_reference(row, d)
    print("L1           %-16s flagged share %.2e (cap %.0e)  loss %.6f  s %.4f" % (name, ref["share"], K.FLAG_CAP[row["math"]], ref["loss"], ref["s_loss"]))
    WORST[("L1 flagged share", row["math"])] = max(WORST.get(("L1 flagged share", row["math"]), (0.0, "")), (ref["share"], name))
    assert ref["share"] <= K.FLAG_CAP[row["math"]], (name, ref["share"])
    for kind in ("fp32",) + (("x3",) if row["math"] == "x3" else ()):
        loss, grad = K.l1_stand_in(row, d, kind)
        worst, wrong, outside, ok = K.l1_check(loss, grad, ref, margin=3.0)
        print("stand-in     %-16s %-5s loss worst %.3f tau  wrong %d  outside %d" % (name, kind, worst, wrong, outside))
        WORST[("L1 loss", kind)] = max(WORST.get(("L1 loss", kind), (0.0, "")), (worst, name))
        assert ok, (name, kind, worst, wrong, outside)
    for m, names in K.MUTANT_ROWS.items():
        if name in names:
            mut = K.l1_reference(row, d, m)
            worst, wrong, outside, ok = K.l1_check(mut["loss"], mut["grad"], ref)
            assert not ok
            _note(m, float("inf") if (wrong or outside) else worst, name)


def test_zz_margins_and_worst_ratios():
    for m, (v, name) in sorted(MARGINS.items()):
        print("margin  %-76s %.1e  %s" % (m, v, name))
    for k, (w, name) in sorted(WORST.items(), key=str):
        print("worst   %-32s %.3e  %s" % (k, w, name))
    if len(MARGINS) == len(K.MUTANT_ROWS) + len(K.MUTANT_ROWS_RMS):      # (the whole file ran)
        assert min(v for v, _ in MARGINS.values()) >= K.MIN_MARGIN
