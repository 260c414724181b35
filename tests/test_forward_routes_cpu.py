"""The forward route table (tests/forward_routes.py) is whole -- every row has its recorded facts, every route the dispatch has is in it --
and the library's workspace function (host code) gives each row's recorded size; the element bound of the fp64 test of the same rows
(tests/test_gpu_forward_fp64.py) holds for CPU stand-ins of the kernels and rejects small changes to the reference.  Runs without a GPU."""
import pytest

import forward_ref as FR
import forward_routes as R
from elem_bound import TAU_BF16X3, TAU_FP32, bound


def test_every_row_has_facts_and_every_route_a_row():
    assert [r["id"] for r in R.ROWS] == list(R.FACTS) and len(set(R.FACTS)) == len(R.ROWS)
    labels = [f[0] for f in R.FACTS.values()]
    missing = [want for want in R.REQUIRED_LABELS if want not in labels]
    assert not missing, missing
    reduced = {lab for lab in labels if lab.startswith("igemm_f32<") and lab.endswith(" + split-K reduce")}
    assert len(reduced) >= 2, reduced
    for label, launches, wsb, sha in R.FACTS.values():
        assert len(sha) == 64 and set(sha) <= set("0123456789abcdef"), sha
        assert launches == (2 if label.endswith(" + split-K reduce") else 1) and wsb >= 0
        assert wsb > 0 or not label.endswith(" + split-K reduce")   # slabs come out of the workspace


def test_workspace_bytes_of_every_row():
    got = {r["id"]: R.workspace_bytes(r) for r in R.ROWS}
    assert got == {k: f[2] for k, f in R.FACTS.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# The element bound of tests/test_gpu_forward_fp64.py discriminates: on three rows of the table, CPU stand-ins of the kernels hold it
# with a 3x margin, and it rejects the fp64 reference after each of four small changes.
# ---------------------------------------------------------------------------------------------------------------------------------
# one `down` at K = 512 (fp32 operands, split inside the kernel), the two-K-halves row at K = 2048, one `up` with a skip source
DISCRIMINATION_ROWS = ("x3.t208.plain", "x3.khalves", "up.n64.m57k.skip")
# 32-channel groups (one tap x 32 channels: 32 consecutive k of the packed weight, the unit of the split32 layout) multiplied hi-only
# by the last mutant.  Measured on the CPU with the whole tensor hi-only: 5e-3 .. 1.4e-2 * s; one group of the K / 32 (16, 64 and -- per
# output pixel of the transposed conv, which sums four taps -- 8) moves the worst element by 3.8e-3, 2.1e-3 and 5.7e-3 * s: one
# group clears TAU_BF16X3 = 2e-4 on every one of the three rows, so none of them needs more.  (Stand-ins, same run: fp32 conv 1.9e-6 ..
# 2.8e-6, split products 1.4e-5 on the split32 rows -- whose reference starts from hi + lo -- and 2.3e-5 on the fp32-operand row.)
HI_ONLY_GROUPS = {"x3.t208.plain": 1, "x3.khalves": 1, "up.n64.m57k.skip": 1}


def tap_contribution(row, x, w, kh, kw, c0, c1):
    """What kernel tap (kh, kw) over input channels [c0, c1) adds to the row's sums z (NCHW x, torch-layout w, any dtype): a 1x1 conv
    over the input pixels the tap reads, placed at the output pixels it feeds (test_tap_contributions_add_up checks it against conv)."""
    import torch
    import torch.nn.functional as F
    if row["kind"] == "up":    # output pixel (2i - 1 + kh, 2j - 1 + kw) reads input pixel (i, j)
        B, _, H, W = x.shape
        t = F.conv2d(x[:, c0:c1], w[c0:c1, :, kh, kw].t()[:, :, None, None])
        out = torch.zeros(B, w.shape[1], 2 * H, 2 * W, dtype=x.dtype)
        i0, i1, j0, j1 = int(kh == 0), H - int(kh == 3), int(kw == 0), W - int(kw == 3)
        out[:, :, 2 * i0 - 1 + kh:2 * i1 - 2 + kh:2, 2 * j0 - 1 + kw:2 * j1 - 2 + kw:2] = t[:, :, i0:i1, j0:j1]
        return out
    s, p = (2, 1) if row["kind"] == "down" else (1, 1)
    _, _, Ho, Wo, _, _, _ = FR.geometry(row)
    xp = F.pad(x[:, c0:c1], (p, p, p, p))
    return F.conv2d(xp[:, :, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s], w[:, c0:c1, kh:kh + 1, kw:kw + 1])


def replicate_top_row(row, x, w, z):
    """z with output row 0 computed as if the padding above the image replicated input row 0 (zero padding everywhere else)."""
    import torch
    import torch.nn.functional as F
    out = z.clone()
    if row["kind"] == "up":    # output row 0 reads input row -1 through kernel row 3
        out[:, :, 0:1] += F.conv_transpose2d(x[:, :, 0:1], w[:, :, 3:4, :], None, 2, (0, 1))
    else:
        assert row["kind"] == "down"
        top = F.pad(x[:, :, 0:3], (1, 1, 0, 0))
        out[:, :, 0:1] = F.conv2d(torch.cat((top[:, :, 0:1], top), 2), w, None, 2, 0)
    return out


def test_tap_contributions_add_up():
    """The helpers above on tiny layers: the taps' contributions sum to the conv, and the replicate-padded row is torch's."""
    import torch
    import torch.nn.functional as F
    for kind, H, W in (("down", 3, 5), ("up", 3, 5), ("c3", 4, 3)):
        row = dict(id="tiny." + kind, kind=kind, B=2, H=H, W=W, C0=32, C1=32 if kind == "up" else 0, N=16, math="fp32", split=0)
        x, x2, w, _, _ = FR.data(row)
        x, w = FR.sources(row, x, x2).double(), w.double()
        z = FR.conv(row, x, w)
        kh_n, kw_n = FR.geometry(row)[6]
        total = sum(tap_contribution(row, x, w, kh, kw, c0, c0 + 32) for kh in range(kh_n) for kw in range(kw_n) for c0 in range(0, x.shape[1], 32))
        assert float((total - z).abs().max()) < 1e-12 * float(z.abs().max()), kind
        if kind == "down":
            want = F.conv2d(F.pad(x, (0, 0, 1, 0), mode="replicate"), w, None, 2, (0, 1))[:, :, 0:1]
            got = replicate_top_row(row, x, w, z)
            assert float((got[:, :, 0:1] - want).abs().max()) < 1e-12 and torch.equal(got[:, :, 1:], z[:, :, 1:])
        if kind == "up":       # a transposed conv over the image with row 0 repeated above it, cropped to the image's own output rows
            want = F.conv_transpose2d(torch.cat((x[:, :, 0:1], x), 2), w, None, 2, 1)[:, :, 2:3]
            got = replicate_top_row(row, x, w, z)
            assert float((got[:, :, 0:1] - want).abs().max()) < 1e-12 and torch.equal(got[:, :, 1:], z[:, :, 1:])


@pytest.mark.parametrize("row_id", DISCRIMINATION_ROWS)
def test_bound_holds_for_stand_ins_and_rejects_mutants(row_id):
    import torch
    row = next(r for r in R.ROWS if r["id"] == row_id)
    x, x2, w, scale, shift = FR.data(row)
    z, r, s = FR.reference(row, x, x2, w, scale, shift)
    xs, ws = FR.sources(row, x, x2), w
    if row["split"]:            # hi + lo is an fp32 value (a multiple of the fp32 ulp of x below 2 |x|)
        xs, ws = FR.seen(row, xs).float(), FR.seen(row, ws).float()
    # stand-ins of the kernel: a plain fp32 convolution, and the three split products summed in fp32
    plain = FR.epilogue(row, FR.conv(row, xs, ws), scale, shift)
    (xh, xl), (wh, wl) = FR.hi_lo(xs), FR.hi_lo(ws)
    x3 = FR.epilogue(row, FR.conv(row, xh, wh) + FR.conv(row, xh, wl) + FR.conv(row, xl, wh), scale, shift)
    for name, g, tau in (("fp32 conv", plain, TAU_FP32), ("hi*hi + hi*lo + lo*hi", x3, TAU_BF16X3)):
        worst, sc, ok = bound(g, r, s, tau / 3)
        print("%-18s stand-in %-22s worst |g-r|/s %.2e  scale-1 %+.1e" % (row_id, name, worst, sc - 1.0))
        assert ok, (row_id, name, worst, sc)
    # mutants of the fp64 reference
    xx, ww = FR.seen(row, FR.sources(row, x, x2)), FR.seen(row, w)
    C = xx.shape[1]
    groups = [(kh, kw, c0) for kh in (1, 2) for kw in (1, 2) for c0 in range(0, C, 32)][:HI_ONLY_GROUPS[row_id]]   # interior taps first
    lo_terms = sum(tap_contribution(row, xx, ww, kh, kw, c0, c0 + 32)
                   - tap_contribution(row, FR.hi_lo(xs)[0].double(), FR.hi_lo(ws)[0].double(), kh, kw, c0, c0 + 32) for kh, kw, c0 in groups)
    mutants = {
        "tap (0, 0) dropped": z - tap_contribution(row, xx, ww, 0, 0, 0, C),
        "scaled by 1 - 1/8": z * (1.0 - 1.0 / 8),
        "top border row with replicate padding": replicate_top_row(row, xx, ww, z),
        "%d group(s) of 32 channels hi-only" % len(groups): z - lo_terms,
    }
    sc64, sh64 = (scale.double(), shift.double()) if scale is not None else (None, None)
    for what, zm in mutants.items():
        worst, sc, ok = bound(FR.epilogue(row, zm, sc64, sh64), r, s, TAU_BF16X3)   # (the wider of the two bounds: TAU_FP32 rejects what it rejects)
        print("%-18s mutant   %-40s worst |g-r|/s %.2e  scale-1 %+.1e" % (row_id, what, worst, sc - 1.0))
        assert not ok and worst > TAU_BF16X3, (row_id, what, worst, sc)
