"""Restatement of the weight-gradient dispatch of csrc/conv_bwd.hip and its kernel families' rules (TEST INFRASTRUCTURE) and the table of gradient test rows.

``wgrad_cfg`` / ``wgrad_splits`` / ``route`` restate, in plain Python, the block shape, split count and reduce / epilogue kernel the
library picks for a launch (wgrad_tiled.hip: wgrad_cfg; conv_bwd.hip: wgrad_splits, conv_wgrad_f32; wgrad_reduce.hip: wgrad_finish).  ``ROWS`` is the table the GPU test
tests/test_gpu_grad_routes.py runs against fp64; tests/test_grad_routes_cpu.py checks, without a GPU, that the table reaches every
route cell below and that the library's workspace sizes agree with the restated split counts (a dispatch change that moves a row to
another route then fails on a CPU box).
"""
WK, WM = 128, 32   # k sub-tile, pixels per reduction chunk

INSTANTIATIONS = ("<128,1,2>", "<64,2,1>", "<64,1,2>", "<32,1,2>", "<32,2,1>", "<32,3,1>")
S_CLASSES = ("S=1", "2<=S<8", "8<S<16,S%8!=0", "S>=16,S%4!=0")
EDGE_CELLS = ("ragged M tail (M%32!=0, S>1)", "padding columns (K%128!=0)", "two-source convT, source switch inside a k sub-tile",
              "knob 12: two k sub-tiles", "knob 12 = -1: three k sub-tiles", "knob 25: 64-wide small-M block", "knob 25 = -1: 128-wide block")
EPILOGUE_CELLS = ("packed reduce, one sum per element (S<16)", "packed reduce, quarter sums (S>=16)",
                  "torch layout <false>", "torch layout <true>", "torch layout, padded channels, gy=1", "torch layout, padded channels, gy>1",
                  "convT reduce-unpack <false>", "convT reduce-unpack <true>")


def cdiv(a, b):
    return (a + b - 1) // b


def wgrad_cfg(N, K, M=1 << 30, knob12=0, knob25=0):
    """(bng, kt, ktiles): n extent of a block, 128-wide k sub-tiles per block, blocks along k."""
    kt128 = cdiv(K, WK)
    bng = 128 if N > 64 else (64 if N > 32 else 32)
    if M <= 1024 and N > 64 and K <= 2048 and knob25 >= 0:
        bng = 64
    if bng == 32:
        kt = 3 if kt128 >= 3 else kt128
    elif bng == 64:
        kt = 2 if (kt128 >= 2 and N <= 64) else 1
    else:
        kt = 1
    if bng == 32 and kt == 3 and knob12 >= 0 and cdiv(kt128, 2) * 2 < cdiv(kt128, 3) * 3:
        kt = 2
    return bng, kt, cdiv(kt128, kt)


def wgrad_splits(M, N, K, knobs=None, row3x3=False):
    knobs = knobs or {}
    bng, _kt, ktiles = wgrad_cfg(N, K, M, knobs.get(12, 0), knobs.get(25, 0))
    tiles = cdiv(N, bng) * ktiles
    chunks = cdiv(M, WM)
    target = knobs[11] if knobs.get(11, 0) > 0 else (768 if row3x3 else 512)
    S = cdiv(target, tiles)
    S = min(S, chunks // 4, 1024)
    return max(S, 1)


def geometry(row):
    """(M, N, K, Ctot, quad, torch_ci) of the row's weight-gradient launch (M: pixels of ONE phase for a transposed conv)."""
    op, B, H, W, C0, C1, Co, k, s, p = (row[f] for f in ("op", "B", "H", "W", "C0", "C1", "Co", "k", "s", "p"))
    Ctot = C0 + C1
    if op == "convT":
        return B * H * W, Co, 4 * Ctot, Ctot, True, 0
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    torch_ci = 0 if op == "wgrad" else row.get("ci", Ctot)
    return B * Ho * Wo, Co, k * k * Ctot, Ctot, False, torch_ci


def is_row3x3(row):
    """The image-row 3x3 kernels' shapes (wgrad_row3x3.hip wgrad_row3x3_rule): not a route of this table (tests/wgrad_routes.py pins them)."""
    return (row["op"] != "convT" and row["k"] == 3 and row["s"] == 1 and row["p"] == 1 and row["C0"] == 32 and row["C1"] == 0 and
            row["W"] == 32 and row["Co"] <= 32 and row["Co"] % 4 == 0)


def route(row):
    """The launch as the library would make it: instantiation, S, reduce kernel, torch-layout tap spread gy, workspace bytes."""
    M, N, K, Ctot, quad, torch_ci = geometry(row)
    knobs = row.get("knobs", {})
    bng, kt, ktiles = wgrad_cfg(N, K, M, knobs.get(12, 0), knobs.get(25, 0))
    S = wgrad_splits(M, N, K, knobs)
    inst = "<%d,%d,%d>" % (bng, kt, 2 if (bng == 128 or (bng == 64 and kt == 1) or (bng == 32 and kt == 1)) else 1)
    ntap = K // Ctot
    gy = 1
    if quad:
        reduce = "convT reduce-unpack <%s>" % ("true" if S >= 16 else "false")
    elif torch_ci > 0:
        gt = N * cdiv(torch_ci, 16)
        tgroups = cdiv(ntap, 16)
        gy = 1 if (gt >= 512 or tgroups == 1) else min(tgroups, 8)
        reduce = "torch layout <%s>" % ("true" if S >= 16 else "false")
    else:
        reduce = "packed reduce, quarter sums (S>=16)" if S >= 16 else "packed reduce, one sum per element (S<16)"
    Kpad = cdiv(K, WK) * WK
    ws = S * N * Kpad * 4
    if quad:
        ws = 4 * ws + 4 * N * K * 4
    return dict(inst=inst, bng=bng, kt=kt, ktiles=ktiles, S=S, M=M, N=N, K=K, Kpad=Kpad, reduce=reduce, gy=gy, workspace=ws,
                quad=quad, torch_ci=torch_ci, Ctot=Ctot)


def s_class(S):
    if S == 1:
        return "S=1"
    if 2 <= S < 8:
        return "2<=S<8"
    if 8 < S < 16 and S % 8:
        return "8<S<16,S%8!=0"
    if S >= 16 and S % 4:
        return "S>=16,S%4!=0"
    return None


def cells(row):
    """Every cell of the coverage lists above that the row's launch reaches."""
    r = route(row)
    out = set()
    sc = s_class(r["S"])
    if sc:
        out.add((r["inst"], sc))
    if r["M"] % WM and r["S"] > 1:
        out.add(EDGE_CELLS[0])
    if r["K"] % WK:
        out.add(EDGE_CELLS[1])
    if r["quad"] and row["C1"] > 0 and row["C0"] % WK:
        out.add(EDGE_CELLS[2])
    kt128 = cdiv(r["K"], WK)
    if r["bng"] == 32 and kt128 >= 3 and cdiv(kt128, 2) * 2 < cdiv(kt128, 3) * 3:   # the shapes knob 12 decides
        out.add(EDGE_CELLS[3] if r["kt"] == 2 else EDGE_CELLS[4])
    if r["M"] <= 1024 and r["N"] > 64 and r["K"] <= 2048:                             # the shapes knob 25 decides
        out.add(EDGE_CELLS[5] if r["bng"] == 64 else EDGE_CELLS[6])
    out.add(r["reduce"])
    if r["torch_ci"] and r["torch_ci"] < r["Ctot"]:
        out.add(EPILOGUE_CELLS[5] if r["gy"] > 1 else EPILOGUE_CELLS[4])
    return out


def all_cells():
    return {(i, s) for i in INSTANTIATIONS for s in S_CLASSES} | set(EDGE_CELLS) | set(EPILOGUE_CELLS)


def _row(id_, op, B, H, W, C0, C1, Co, k=1, s=1, p=0, slope=1.0, bias=False, ci=None, knobs=None, dx=True, shipped=None, S=None):
    """S: the split count to run at, set through knob 11 (the block-count target: S = ceil(target / tiles), so target = S * tiles changes the
    split count and nothing else)."""
    r = dict(id=id_, op=op, B=B, H=H, W=W, C0=C0, C1=C1, Co=Co, k=k, s=s, p=p, slope=slope, bias=bias, knobs=dict(knobs or {}), dx=dx,
             shipped=shipped, S=S)
    if ci is not None:
        r["ci"] = ci
    if S is not None:
        M, N, K = geometry(r)[:3]
        bng, _kt, ktiles = wgrad_cfg(N, K, M, r["knobs"].get(12, 0), r["knobs"].get(25, 0))
        r["knobs"][11] = S * cdiv(N, bng) * ktiles
    return r


def _passive_rows(B, net):
    """One network of the passive step (PassiveSepEncCNN / PassiveSepDecCNN training forward, separator_cnn.py) at B rows, 32 frames."""
    bin_ = net == "binSep"
    c_in, ci0 = (36, 33) if bin_ else (32, 32)   # binSep: 32 slice channels + the class plane, padded to 36 (sep_slice_input_plane)
    rows = []
    enc = [(c_in, 64, 32), (64, 128, 16), (128, 256, 8), (256, 512, 4), (512, 512, 2)]
    for i, (ci, co, h) in enumerate(enc):
        rows.append(_row("%s.enc%d.B%d" % (net, i, B), "conv", B, h, h, ci, 0, co, 4, 2, 1, ci=ci0 if i == 0 else ci, dx=i > 0,
                         shipped="passive.%s.enc%d" % (net, i)))
    out_a = 32 if bin_ else 16
    dec = [(512, 0, 512, 1), (512, 512, 256, 2), (256, 256, 128, 4), (128, 128, 64, 8), (64, 64, out_a, 16)]
    for i, (c0, c1, co, h) in enumerate(dec):
        rows.append(_row("%s.dec%d.B%d" % (net, i, B), "convT", B, h, h, c0, c1, co, shipped="passive.%s.dec%d" % (net, i)))
    rows.append(_row("%s.head.B%d" % (net, B), "conv", B, 32, 32, out_a, 0, out_a, 1, 1, 0, bias=True, dx=True, shipped="passive.%s.head" % net))
    return rows


def _policy_rows(B):
    """The policy encoders of update_pol (AudioCNN, VisualCNN: rl/models/audio_cnn.py, visual_cnn.py) at B rows: convs + full-spatial Linear."""
    return [
        _row("audio.conv0.B%d" % B, "conv", B, 32, 32, 32, 0, 32, 8, 4, 0, slope=0.0, bias=True, shipped="policy.audio.conv0"),
        _row("audio.conv1.B%d" % B, "conv", B, 7, 7, 32, 0, 64, 4, 2, 0, slope=0.0, bias=True, shipped="policy.audio.conv1"),
        _row("audio.conv2.B%d" % B, "conv", B, 2, 2, 64, 0, 32, 2, 1, 0, slope=0.0, bias=True, shipped="policy.audio.conv2"),
        _row("audio.fc.B%d" % B, "conv", B, 1, 1, 32, 0, 512, 1, 1, 0, slope=0.0, bias=True, shipped="policy.audio.fc"),
        _row("visual.conv0.B%d" % B, "conv", B, 128, 128, 4, 0, 32, 8, 4, 0, slope=0.0, bias=True, ci=3, shipped="policy.visual.conv0"),
        _row("visual.conv1.B%d" % B, "conv", B, 31, 31, 32, 0, 64, 4, 2, 0, slope=0.0, bias=True, shipped="policy.visual.conv1"),
        _row("visual.conv2.B%d" % B, "conv", B, 14, 14, 64, 0, 32, 3, 1, 0, slope=1.0, bias=True, shipped="policy.visual.conv2"),
        _row("visual.fc.B%d" % B, "conv", B, 12, 12, 32, 0, 512, 12, 1, 0, slope=0.0, bias=True, shipped="policy.visual.fc"),
    ]


def _route_rows():
    """Rows that place each instantiation at each split class (knob 11 = block-count target where no natural shape does), plus the
    edges and epilogues the shipped shapes miss."""
    R = []
    # <128,1,2>: N > 64 (at M <= 1024 only with knob 25 = -1)
    R += [_row("i128.S1", "conv", 2, 8, 8, 64, 0, 128, 3, 1, 1, knobs={25: -1}),                          # M 128: 4 chunks
          _row("i128.S3", "wgrad", 4, 18, 18, 96, 0, 160, 3, 1, 1, S=3),                                  # K 864: padding columns; N 160: two n-blocks
          _row("i128.S11", "conv", 7, 15, 15, 64, 0, 192, 3, 1, 1, slope=0.2, bias=True, S=11),           # M 1575: ragged tail
          _row("i128.S19", "wgrad", 10, 16, 16, 128, 0, 130, S=19)]                                       # N 130: scalar dY tail
    # <64,2,1>: 32 < N <= 64, K > 128
    R += [_row("i64k2.S1", "conv", 3, 6, 6, 32, 0, 48, 3, 1, 1, bias=True),                               # M 108: 4 chunks
          _row("i64k2.S5", "conv", 7, 10, 10, 64, 0, 64, 3, 1, 1, slope=0.0, bias=True, S=5),
          _row("i64k2.S13", "convT", 5, 20, 20, 100, 28, 64, S=13),                                       # C0 100: the source switch inside a sub-tile
          _row("i64k2.S26", "conv", 13, 16, 16, 40, 0, 56, 3, 1, 1, S=26)]                                # K 360
    # <64,1,2>: the small-M 64-wide rule (N > 64, M <= 1024, K <= 2048), or K <= 128 with 32 < N <= 64
    R += [_row("i64k1.S1", "linear", 37, 1, 1, 512, 0, 512),                                              # M 37: 2 chunks
          _row("i64k1.S2", "linear", 280, 1, 1, 1536, 0, 512, bias=True),                                 # the update batch's 1536-wide Linear
          _row("i64k1.S14", "conv", 2000, 1, 1, 96, 0, 48, bias=True, S=14),                              # K 96: one padded sub-tile
          _row("i64k1.S23", "wgrad", 21, 12, 12, 120, 0, 64, S=23)]                                       # M 3024: ragged tail
    # <32,1,2>: N <= 32, K <= 128
    R += [_row("i32k1.S1", "conv", 1, 7, 9, 16, 0, 16, bias=True),
          _row("i32k1.S3", "wgrad", 4, 9, 11, 100, 0, 24, S=3),
          _row("i32k1.S10", "conv", 5, 20, 17, 64, 0, 20, slope=0.0, bias=True, S=10),
          _row("i32k1.S19", "wgrad", 8, 17, 19, 8, 24, 32, S=19)]                                         # two sources, packed layout
    # <32,2,1>: N <= 32, two sub-tiles (K in (128, 256], or K in (384, 512] by the knob-12 rule)
    R += [_row("i32k2.S1", "conv", 2, 5, 5, 24, 0, 32, 3, 1, 1, bias=True),                               # K 216
          _row("i32k2.S3", "convT", 2, 16, 16, 64, 64, 16, S=3),                                          # the mono decoder's last stage in small
          _row("i32k2.S9", "wgrad", 8, 24, 24, 128, 0, 28, 2, 2, 0, S=9),                                 # K 512: knob 12 -> two sub-tiles
          _row("i32k2.S18", "conv", 9, 16, 16, 16, 0, 32, 3, 1, 1, slope=0.0, bias=True, S=18)]
    # <32,3,1>: N <= 32, K > 256 where the knob-12 rule does not take two
    R += [_row("i32k3.S1", "conv", 2, 4, 4, 36, 0, 32, 3, 1, 1),                                          # K 324
          _row("i32k3.S4", "wgrad", 8, 16, 16, 128, 0, 32, 2, 2, 0, knobs={12: -1}, S=4),                 # K 512 with knob 12 = -1: three sub-tiles
          _row("i32k3.S15", "conv", 12, 13, 13, 32, 0, 20, 3, 1, 1, slope=0.2, S=15),                     # K 288, M 2028: ragged tail
          _row("i32k3.S18", "conv", 36, 17, 17, 72, 0, 32, 4, 2, 1, bias=True, S=18)]                     # K 1152: nine sub-tiles, three per block
    # edges / epilogues the rows above and the shipped shapes miss
    R += [_row("edge.small_m_off", "linear", 280, 1, 1, 1536, 0, 512, knobs={25: -1}),                    # 128-wide blocks at M 280
          _row("edge.pad_gy", "conv", 11, 40, 40, 4, 0, 32, 8, 4, 0, slope=0.0, bias=True, ci=3)]         # VisualCNN conv0's class at S 7, gy 4
    return R


ROWS = _route_rows() + _passive_rows(64, "binSep") + _passive_rows(64, "bin2mono") + _policy_rows(280) + _policy_rows(37)
ROWS_BY_ID = {r["id"]: r for r in ROWS}
SHIPPED = (["passive.%s.%s" % (n, l) for n in ("binSep", "bin2mono") for l in ("enc0", "enc1", "enc2", "enc3", "enc4", "dec0", "dec1", "dec2",
                                                                                   "dec3", "dec4", "head")] +
           ["policy.%s.%s" % (n, l) for n in ("audio", "visual") for l in ("conv0", "conv1", "conv2", "fc")])

# bias-gradient rows (m2h_bias_grad / m2h_act_bwd_bias): (M, N, slope) on both sides of the one-stage limit (M <= 1024), narrow N that
# divides 64 (the narrow partial kernel) and narrow N that does not
BIAS_ROWS = [(280, 512, 1.0), (37, 20, 0.0), (1024, 48, 0.2), (65536, 32, 1.0), (5000, 16, 0.0), (3001, 20, 1.0), (4099, 96, 0.2), (20000, 2, 0.0)]
