"""GPU: every row of the forward route table (tests/forward_routes.py: one row per side of every threshold conv_igemm_f32's dispatch
reads) element by element against CPU float64 -- the table's SHA-256 facts prove that nothing changed, this proves the values are right.

Per row: normal data from the row's own seed in the torch layouts, packed by the library's packers (forward_routes.run_on: so the
packers and the sub-pixel phase / tap map are under the reference too); the launch is the route the hash pins (label, launches and
workspace bytes equal the recorded facts: the dispatch reads shapes only); then, with r and s of tests/forward_ref.py,
  |g_e - r_e| <= tau * s_e for every element,   <g, r> / <r, r> = 1 +- tau,   rel-L1 < 5 tau
(tests/elem_bound.py; tests/test_forward_routes_cpu.py proves without a GPU that this rejects a dropped tap, a (1 - 1/8) scale, one
border row padded wrongly and one 32-channel group multiplied hi-only).  tau = TAU_FP32 for fp32 rows, TAU_BF16X3 for bf16x3 rows.

FORMS: epilogue and operand forms no row of the table holds -- class plane, de-sliced output, fused head, strided destination,
split32 output, a ragged two-row image -- under the same bound, in fp32, bf16x3 and bf16x3 on split32 operands where the form allows.

The last parametrised test puts the two forms the U-Net runner uses on its large stages -- fused head, split32 output -- on rows of the
table itself, where they reach the transposed-conv kernels' head epilogue and the split32 stores of the LDS-DMA, shared-patch and
four-phase engines."""
import pytest
import torch

import forward_ref as FR
import forward_routes as R
import m2h_oracle as O
from elem_bound import TAU_BF16X3, TAU_FP32, bound
from test_gpu_patch import unsplit32

pytestmark = pytest.mark.gpu

# Measured on an MI355X (worst |g - r| / s over the table and the forms, printed per row with -s; test_zz_report sums it up per label and
# per arithmetic): fp32 5.5e-6 (igemm_f32<128,128>, n72.t256; the skinny kernels 1.2e-6, the image-row kernels 3.8e-6), bf16x3 on fp32
# operands 2.4e-5 (every engine within 1.9e-5 .. 2.4e-5), bf16x3 on split32 operands 1.6e-5 (the reference starts from hi + lo), with
# split32 output 3.6e-5 (the output's own rounding is up to 2^-18 |r|, and |r| reaches 8 s over 4 M elements).  The forms at the small
# shapes: fp32 1.1e-6, bf16x3 2.0e-5.  The bounds sit 3.6x (fp32) and 5.5x - 8x (bf16x3) above; no row needed a kernel fix.
TAU = {"fp32": TAU_FP32, "bf16x3": TAU_BF16X3}
WORST = {}   # case id -> (label, arithmetic, worst ratio)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _check(case, row, label, g, r, s):
    """The three assertions on one output (g from the GPU; r, s float64), recorded for the report."""
    tau = TAU[row["math"]]
    g = g.double().cpu()
    worst, scale, ok = bound(g, r, s, tau)
    rl1 = O.rel_l1(g, r)
    WORST[case] = (label, row["math"] + (" split32" if row["split"] else ""), worst)
    print("%-24s %-6s %-40s worst |g-r|/s %.2e  scale-1 %+.1e  rel-L1 %.1e" % (case, row["math"], label, worst, scale - 1.0, rl1))
    assert ok, (case, label, worst, scale)
    assert rl1 < 5 * tau, (case, label, rl1)


@pytest.mark.parametrize("row", R.ROWS, ids=[r["id"] for r in R.ROWS])
def test_forward_row_matches_fp64(row):
    x, x2, w, scale, shift = FR.data(row)
    out, label, launches, wsb = R.run_on(row, _dev(), x, x2, w, scale, shift)
    assert (label, launches, wsb) == R.FACTS[row["id"]][:3]     # the route the recorded hash pins
    _, r, s = FR.reference(row, x, x2, w, scale, shift)
    _check(row["id"], row, label, out, FR.nhwc(r), FR.nhwc(s))


# ---------------------------------------------------------------------------------------------------------------------------------
# Forms the table does not hold (no hash facts), at the smallest shapes that still cross a tile edge
# ---------------------------------------------------------------------------------------------------------------------------------
def _row(id_, kind, B, H, W, C0, C1, N):
    return dict(id=id_, kind=kind, B=B, H=H, W=W, C0=C0, C1=C1, N=N)


FORMS = {
    # the target-class plane of the first encoder stage: 8 x 8 outputs hold all nine border classes; odd batch
    "cls": _row("form.cls", "down", 3, 8, 8, 32, 0, 64),
    # OUT_DESLICE of a 1x1 conv over 4 x 8 pixels: N / 16 = 2 and 1 output channels
    "deslice.n32": _row("form.deslice.n32", "c1", 2, 4, 8, 32, 0, 32),
    "deslice.n16": _row("form.deslice.n16", "c1", 2, 4, 8, 32, 0, 16),
    # the last decoder stage with the fused 1x1 head (no workspace), two sources
    "head.n16": _row("form.head.n16", "up", 2, 4, 8, 32, 32, 16),
    "head.n32": _row("form.head.n32", "up", 2, 4, 8, 32, 32, 32),
    # a Linear over 14 rows into a column block of a wider matrix (ldc > N)
    "ldc": _row("form.ldc", "lin", 14, 1, 1, 512, 0, 128),
    # FMT_DST_SPLIT (split32 operands only)
    "dst_split.down": _row("form.dst_split.down", "down", 3, 8, 8, 32, 0, 64),
    "dst_split.up": _row("form.dst_split.up", "up", 2, 4, 8, 32, 32, 32),
    # an odd batch of two-row images: 1 x 8 outputs, half of every window in the padding
    "ragged": _row("form.ragged", "down", 3, 1, 8, 128, 0, 256),
}
OPERANDS = {"fp32": ("fp32", 0), "bf16x3": ("bf16x3", 0), "bf16x3.split32": ("bf16x3", 1)}
FORM_CASES = [(f, o) for f in FORMS for o in OPERANDS if not f.startswith("dst_split") or o == "bf16x3.split32"]
# The two forms the U-Net runner uses on its large stages, on rows of the table itself: at the small shapes above they reach the
# register engine only, here the transposed-conv kernels' own head epilogue and the split32 stores of the LDS-DMA, shared-patch and
# four-phase engines (with and without their split-K reduce).  The form does not move the route: the label is the row's recorded one.
TABLE_FORM_CASES = [("head", "up.n16.m32k"), ("head", "up.n32.m32k.split"), ("head", "up.n32.m57k.split"),
                    ("dst_split", "x3.t208.split"), ("dst_split", "x3.t224.split"), ("dst_split", "x3.t224.c3"), ("dst_split", "x3.khalves"),
                    ("dst_split", "up.patch64.t224"), ("dst_split", "up.n64.m57k.skip")]
SENTINEL = -12345.678


@pytest.mark.parametrize("form,operands", FORM_CASES, ids=["%s-%s" % c for c in FORM_CASES])
def test_form_matches_fp64(form, operands):
    row = dict(FORMS[form], math=OPERANDS[operands][0], split=OPERANDS[operands][1])
    _run_form(form.split(".")[0], row, "%s-%s" % (row["id"], operands))


@pytest.mark.parametrize("kind,row_id", TABLE_FORM_CASES, ids=["%s-%s" % c for c in TABLE_FORM_CASES])
def test_form_on_table_row_matches_fp64(kind, row_id):
    row = next(r for r in R.ROWS if r["id"] == row_id)
    label = _run_form(kind, row, "form.%s-%s" % (kind, row_id))
    assert label == R.FACTS[row_id][0]


def _run_form(kind, row, case):
    """One form on one row against float64; returns the label of the kernel that ran."""
    dev = _dev()
    x, x2, w, scale, shift = FR.data(row, extra_in=1 if kind == "cls" else 0)
    g = torch.Generator().manual_seed(len(case))
    if kind == "cls":
        # reference: the 33-channel conv with the plane (target_class + 1, constant over each image) as a real channel
        cls_val = torch.randint(1, 4, (row["B"],), generator=g).float()
        out, label, _, _ = R.run_on(row, dev, x, None, w, scale, shift, cls_val=cls_val)
        plane = cls_val.view(-1, 1, 1, 1).expand(-1, 1, x.shape[2], x.shape[3])
        _, r, s = FR.reference(row, x, plane, w, scale, shift)   # (cls_val is a small integer: hi + lo of a split row leaves it as it is)
        _check(case, row, label, out, FR.nhwc(r), FR.nhwc(s))
    elif kind == "deslice":
        out, label, _, _ = R.run_on(row, dev, x, x2, w, scale, shift, deslice=True)
        _, r, s = FR.reference(row, x, x2, w, scale, shift)
        _check(case, row, label, out, O.deslice_freq(r), O.deslice_freq(s))
    elif kind == "head":
        # out_j = sum_n head_w[j][n] * y_n + head_b[j] on the stage's output y, stored de-sliced.  The terms summed into out_j are the
        # stage's own products times head_w[j][n], so s_j = sqrt(sum_n head_w[j][n]^2 * s_n^2) + |head_b[j]|: the same construction
        # one level up (the head's fp32 rounding of sum_n is 2^-24 of it: far below tau * s_j).
        N = row["N"]
        hw, hb = torch.randn(N, N, generator=g) * (2.0 / N) ** 0.5, torch.randn(N, generator=g) * 0.1
        out, label, _, wsb = R.run_on(row, dev, x, x2, w, scale, shift, head=(hw, hb))
        assert wsb == 0
        _, y, sy = FR.reference(row, x, x2, w, scale, shift)
        r = torch.einsum("jn,bnhw->bjhw", hw.double(), y) + hb.double().view(1, -1, 1, 1)
        s = torch.einsum("jn,bnhw->bjhw", hw.double() ** 2, sy ** 2).sqrt() + hb.double().abs().view(1, -1, 1, 1)
        _check(case, row, label, out, O.deslice_freq(r), O.deslice_freq(s))
    elif kind == "ldc":
        M, N, ldc, c0 = row["B"], row["N"], 256, 64
        wide = torch.full((M, ldc), SENTINEL, device=dev)
        out, label, _, _ = R.run_on(row, dev, x, x2, w, scale, shift, dst=wide[:, c0:c0 + N], ldc=ldc)
        _, r, s = FR.reference(row, x, x2, w, scale, shift)
        got = wide.cpu()
        _check(case, row, label, got[:, c0:c0 + N], r.reshape(M, N), s.reshape(M, N))
        keep = torch.full((M, ldc), SENTINEL)
        outside = torch.ones(M, ldc, dtype=torch.bool)
        outside[:, c0:c0 + N] = False
        assert torch.equal(got.view(torch.int32)[outside], keep.view(torch.int32)[outside])   # bit for bit
    elif kind == "dst_split":
        out, label, _, _ = R.run_on(row, dev, x, x2, w, scale, shift, dst_split=True)
        _, r, s = FR.reference(row, x, x2, w, scale, shift)
        # hi + lo keeps 16 to 17 bits of the output: its rounding, 2^-17 |r|, joins s
        _check(case, row, label, unsplit32(out.cpu()), FR.nhwc(r), FR.nhwc(s + 2.0 ** -17 * r.abs()))   # (hi + lo is an fp32 value)
    else:
        assert kind == "ragged"
        out, label, _, _ = R.run_on(row, dev, x, x2, w, scale, shift)
        _, r, s = FR.reference(row, x, x2, w, scale, shift)
        _check(case, row, label, out, FR.nhwc(r), FR.nhwc(s))
    return label


def test_zz_report():
    """(summary of the runs above: worst |g - r| / s per row, per kernel label and per arithmetic, for the record; when the whole table
    ran, every label the table must reach has been checked against float64)"""
    for case, (label, math, worst) in WORST.items():
        print("row   %-32s %-14s %-40s %.2e" % (case, math, label, worst))
    by_label, by_math = {}, {}
    for label, math, worst in WORST.values():
        by_label[label] = max(by_label.get(label, 0.0), worst)
        by_math[math] = max(by_math.get(math, 0.0), worst)
    for label, worst in sorted(by_label.items()):
        print("label %-40s worst |g-r|/s %.2e" % (label, worst))
    for math, worst in sorted(by_math.items()):
        print("math  %-14s worst |g-r|/s %.2e" % (math, worst))
    if all(r["id"] in WORST for r in R.ROWS):
        missing = [want for want in R.REQUIRED_LABELS if want not in by_label]
        assert not missing, missing
