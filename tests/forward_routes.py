"""Route table of the forward dispatch (conv_igemm_f32 in csrc/conv_igemm.hip): one row per shape that sits on one side of a threshold
the dispatch reads, with what the library did with it under default knobs -- the label of m2h_last_kernel, the number of launches
the call made and the split-K workspace m2h_conv_igemm_workspace_bytes asked for.  The facts are OBSERVED, not derived: they were
recorded once on an MI355X from the library as it stood before the retired tuning knobs (include/m2h_tuning.h) were removed, and a
refactor of the dispatch must leave every one of them as it is.  Never regenerate them from the code under test; a pull request
that means to change a route changes its row by hand and says why.  The recording run, with the SHA-256 of every row's output and the
kernel trace at both commits, is profiles/forward_routes_parent_vs_branch.txt.

Row geometry (kind):
  down  Conv2d(4, 2, 1) as the U-Net runner issues it (down_args in csrc/api.hip); H x W is the OUTPUT pixel grid
  up    ConvTranspose2d(4, 2, 1) as four sub-pixel phases (up_args); H x W is the INPUT pixel grid, C1 > 0 adds a skip source
  c3    Conv2d(3, 1, 1); H x W is the image
  lin   nn.Linear over B rows of C0 floats (H = W = 1)
  full  a conv whose window is the whole H x W image: one output pixel per sample
M = B * H * W GEMM rows (per phase for `up`); `split` = sources and weights in the split32 layout (bf16x3 only)."""
import ctypes

import torch

# (id, kind, B, H, W, C0, C1, N, math, split), then the observed (label, launches, workspace bytes)
_ROWS = [
    # ---- M <= 16 | 17: the skinny rows kernel | the skinny gather kernel (fp32)
    ("m16.lin", "lin", 16, 1, 1, 512, 0, 128, "fp32", 0),
    ("m17.lin", "lin", 17, 1, 1, 512, 0, 128, "fp32", 0),
    ("m14.lin1536", "lin", 14, 1, 1, 512, 0, 1536, "fp32", 0),        # the wide form (16 columns per block)
    ("m14.full", "full", 14, 4, 4, 32, 0, 64, "fp32", 0),             # full-window conv: one pixel per sample
    ("m280.lin512", "lin", 280, 1, 1, 512, 0, 512, "fp32", 0),        # 32 x 32 blocks
    ("m280.lin1536", "lin", 280, 1, 1, 512, 0, 1536, "fp32", 0),      # 64 x 32 blocks
    # ---- M at 32 | 33, 64 | 65: the 32- / 64- / 128-row tiles of the 128-wide register engine (bf16x3: fp32 takes the gather kernel here)
    ("m32.x3", "lin", 32, 1, 1, 512, 0, 128, "bf16x3", 0),
    ("m33.x3", "lin", 33, 1, 1, 512, 0, 128, "bf16x3", 0),
    ("m64.x3", "lin", 64, 1, 1, 512, 0, 128, "bf16x3", 0),
    ("m65.x3", "lin", 65, 1, 1, 512, 0, 128, "bf16x3", 0),
    # ---- M at 1024 | 1025: the gather kernel's pixel limit (weights of 64 K elements)
    ("m1024.lin", "lin", 1024, 1, 1, 512, 0, 128, "fp32", 0),
    ("m1025.lin", "lin", 1025, 1, 1, 512, 0, 128, "fp32", 0),
    # ---- M at 4096 | 4097: its limit against tiny weights (32 K elements), and the same rows against 64 K
    ("m4096.tiny", "lin", 4096, 1, 1, 512, 0, 64, "fp32", 0),
    ("m4097.tiny", "lin", 4097, 1, 1, 512, 0, 64, "fp32", 0),
    ("m4096.w64k", "lin", 4096, 1, 1, 512, 0, 128, "fp32", 0),
    ("m4097.w64k", "lin", 4097, 1, 1, 512, 0, 128, "fp32", 0),
    # ---- N at 16 | 20, 32 | 36, 64 | 72, 128 (fp32): 64 tiles of 128 rows (split-K) and 256 (none)
    ("n16.t64", "down", 2, 64, 64, 32, 0, 16, "fp32", 0),
    ("n20.t64", "down", 2, 64, 64, 32, 0, 20, "fp32", 0),
    ("n32.t64", "down", 2, 64, 64, 32, 0, 32, "fp32", 0),
    ("n36.t64", "down", 2, 64, 64, 32, 0, 36, "fp32", 0),
    ("n64.t64", "down", 2, 64, 64, 32, 0, 64, "fp32", 0),
    ("n72.t64", "down", 2, 64, 64, 32, 0, 72, "fp32", 0),
    ("n128.t64", "down", 2, 64, 64, 32, 0, 128, "fp32", 0),
    ("n16.t256", "down", 8, 64, 64, 32, 0, 16, "fp32", 0),
    ("n20.t256", "down", 8, 64, 64, 32, 0, 20, "fp32", 0),
    ("n32.t256", "down", 8, 64, 64, 32, 0, 32, "fp32", 0),
    ("n36.t256", "down", 8, 64, 64, 32, 0, 36, "fp32", 0),
    ("n64.t256", "down", 8, 64, 64, 32, 0, 64, "fp32", 0),
    ("n72.t256", "down", 8, 64, 64, 32, 0, 72, "fp32", 0),
    ("n128.t256", "down", 8, 64, 64, 32, 0, 128, "fp32", 0),
    # ---- register-engine tile count at 255 | 256
    ("t255.lin", "lin", 255 * 128, 1, 1, 256, 0, 128, "fp32", 0),
    ("t256.lin", "lin", 256 * 128, 1, 1, 256, 0, 128, "fp32", 0),
    # ---- bf16x3, N = 128: 208 | 224 tiles of 256 rows -- plain, split32 on the 4x4/s2 geometry, split32 on a 3x3/s1 conv
    ("x3.t208.plain", "down", 13, 64, 64, 32, 0, 128, "bf16x3", 0),
    ("x3.t224.plain", "down", 14, 64, 64, 32, 0, 128, "bf16x3", 0),
    ("x3.t208.split", "down", 13, 64, 64, 32, 0, 128, "bf16x3", 1),
    ("x3.t224.split", "down", 14, 64, 64, 32, 0, 128, "bf16x3", 1),
    ("x3.t208.c3", "c3", 13, 64, 64, 32, 0, 128, "bf16x3", 1),
    ("x3.t224.c3", "c3", 14, 64, 64, 32, 0, 128, "bf16x3", 1),
    # ---- two K-halves: 128 tiles, K = 2048
    ("x3.khalves", "down", 8, 64, 64, 128, 0, 128, "bf16x3", 1),
    # ---- the 64-wide shared-patch tile (whole images per 512-row tile): 220 | 224 tiles of 512 rows, as the runner's last-but-one decoder stage
    ("up.patch64.t220", "up", 55, 8, 64, 32, 32, 64, "bf16x3", 1),
    ("up.patch64.t224", "up", 56, 8, 64, 32, 32, 64, "bf16x3", 1),
    ("x3.n64.img4096", "down", 28, 64, 64, 32, 0, 64, "bf16x3", 1),   # 224 tiles, but images larger than a tile: not that engine
    # ---- transposed convs in bf16x3 at M = 32768 | 57344, 64 pixels wide
    ("up.n16.m32k", "up", 8, 64, 64, 32, 0, 16, "bf16x3", 0),
    ("up.n16.m57k", "up", 14, 64, 64, 32, 0, 16, "bf16x3", 0),
    ("up.n64.m32k", "up", 8, 64, 64, 32, 0, 64, "bf16x3", 0),
    ("up.n64.m57k", "up", 14, 64, 64, 32, 0, 64, "bf16x3", 0),
    ("up.n32.m32k.split", "up", 8, 64, 64, 32, 0, 32, "bf16x3", 1),
    ("up.n32.m57k.split", "up", 14, 64, 64, 32, 0, 32, "bf16x3", 1),
    ("up.n64.m32k.split", "up", 8, 64, 64, 32, 0, 64, "bf16x3", 1),
    ("up.n64.m57k.split", "up", 14, 64, 64, 32, 0, 64, "bf16x3", 1),
    ("up.n64.m57k.h28", "up", 32, 28, 64, 32, 0, 64, "bf16x3", 1),    # 28 rows: no power-of-two grid, so not the shared-patch engine
    ("up.n64.m57k.skip", "up", 32, 28, 64, 32, 32, 64, "bf16x3", 1),  # ... with a skip source
    # ---- image-row 3x3: B * H / 4 at 512 | 480
    ("row.b64.n16.fp32", "c3", 64, 32, 32, 32, 0, 16, "fp32", 0),
    ("row.b60.n16.fp32", "c3", 60, 32, 32, 32, 0, 16, "fp32", 0),
    ("row.b64.n32.fp32", "c3", 64, 32, 32, 32, 0, 32, "fp32", 0),
    ("row.b60.n32.fp32", "c3", 60, 32, 32, 32, 0, 32, "fp32", 0),
    ("row.b64.n16.x3", "c3", 64, 32, 32, 32, 0, 16, "bf16x3", 0),
    ("row.b60.n16.x3", "c3", 60, 32, 32, 32, 0, 16, "bf16x3", 0),
    ("row.b64.n32.x3", "c3", 64, 32, 32, 32, 0, 32, "bf16x3", 0),
    ("row.b60.n32.x3", "c3", 60, 32, 32, 32, 0, 32, "bf16x3", 0),
]

# id -> (label of m2h_last_kernel, launches of the call, workspace bytes): as observed, see the module docstring
FACTS = {
    "m16.lin": ("conv_igemm_f32 (skinny rows)", 1, 0),
    "m17.lin": ("conv_igemm_f32 (skinny gather)", 1, 0),
    "m14.lin1536": ("conv_igemm_f32 (skinny rows)", 1, 0),
    "m14.full": ("conv_igemm_f32 (skinny rows)", 1, 14336),
    "m280.lin512": ("conv_igemm_f32 (skinny gather)", 1, 2293760),
    "m280.lin1536": ("conv_igemm_f32 (skinny gather)", 1, 6881280),
    "m32.x3": ("igemm_f32<32,128>", 1, 0),
    "m33.x3": ("igemm_f32<64,128>", 1, 0),
    "m64.x3": ("igemm_f32<64,128>", 1, 0),
    "m65.x3": ("igemm_f32<128,128> + split-K reduce", 2, 133120),
    "m1024.lin": ("conv_igemm_f32 (skinny gather)", 1, 2097152),
    "m1025.lin": ("igemm_f32<128,128> + split-K reduce", 2, 2099200),
    "m4096.tiny": ("conv_igemm_f32 (skinny gather)", 1, 4194304),
    "m4097.tiny": ("igemm_f32<128,64> + split-K reduce", 2, 4195328),
    "m4096.w64k": ("igemm_f32<128,128> + split-K reduce", 2, 8388608),
    "m4097.w64k": ("igemm_f32<128,128> + split-K reduce", 2, 8390656),
    "n16.t64": ("igemm_f32<128,16> + split-K reduce", 2, 2097152),
    "n20.t64": ("igemm_f32<128,32> + split-K reduce", 2, 2621440),
    "n32.t64": ("igemm_f32<128,32> + split-K reduce", 2, 4194304),
    "n36.t64": ("igemm_f32<128,64> + split-K reduce", 2, 4718592),
    "n64.t64": ("igemm_f32<128,64> + split-K reduce", 2, 8388608),
    "n72.t64": ("igemm_f32<128,128> + split-K reduce", 2, 9437184),
    "n128.t64": ("igemm_f32<128,128> + split-K reduce", 2, 16777216),
    "n16.t256": ("igemm_f32<128,16>", 1, 0),
    "n20.t256": ("igemm_f32<128,32>", 1, 0),
    "n32.t256": ("igemm_f32<128,32>", 1, 0),
    "n36.t256": ("igemm_f32<128,64>", 1, 0),
    "n64.t256": ("igemm_f32<128,64>", 1, 0),
    "n72.t256": ("igemm_f32<128,128>", 1, 0),
    "n128.t256": ("igemm_f32<128,128>", 1, 0),
    "t255.lin": ("igemm_f32<128,128> + split-K reduce", 2, 33423360),
    "t256.lin": ("igemm_f32<128,128>", 1, 0),
    "x3.t208.plain": ("igemm_f32<128,128>", 1, 0),
    "x3.t224.plain": ("igemm_f32<256,128> (eight waves)", 1, 0),
    "x3.t208.split": ("igemm_dma<256,128> + split-K reduce", 2, 54525952),
    "x3.t224.split": ("igemm_patch<256,128>", 1, 0),
    "x3.t208.c3": ("igemm_f32<128,128>", 1, 0),
    "x3.t224.c3": ("igemm_dma<256,128>", 1, 0),
    "x3.khalves": ("igemm_patch<256,128> + split-K reduce", 2, 33554432),
    "up.patch64.t220": ("igemm_f32<128,64>", 1, 0),
    "up.patch64.t224": ("igemm_patch<512,64>", 1, 0),
    "x3.n64.img4096": ("igemm_f32<128,64>", 1, 0),
    "up.n16.m32k": ("igemm_convT_tap<16>", 1, 0),
    "up.n16.m57k": ("igemm_convT_tap<16>", 1, 0),
    "up.n64.m32k": ("igemm_convT_tap<64>", 1, 0),
    "up.n64.m57k": ("igemm_convT_tap<64>", 1, 0),
    "up.n32.m32k.split": ("igemm_convT_tap<32>", 1, 0),
    "up.n32.m57k.split": ("igemm_convT_quad<32>", 1, 0),
    "up.n64.m32k.split": ("igemm_convT_quad<64>", 1, 0),
    "up.n64.m57k.split": ("igemm_convT_quad<64>", 1, 0),
    "up.n64.m57k.h28": ("igemm_convT_quad<64>", 1, 0),
    "up.n64.m57k.skip": ("igemm_convT_quad<64>", 1, 0),
    "row.b64.n16.fp32": ("conv_igemm_f32 (image-row 3x3)", 1, 0),
    "row.b60.n16.fp32": ("igemm_f32<128,16>", 1, 0),
    "row.b64.n32.fp32": ("conv_igemm_f32 (image-row 3x3)", 1, 0),
    "row.b60.n32.fp32": ("igemm_f32<128,32>", 1, 0),
    "row.b64.n16.x3": ("conv_igemm_bf16x3 (image-row 3x3)", 1, 0),
    "row.b60.n16.x3": ("igemm_f32<128,16>", 1, 0),
    "row.b64.n32.x3": ("conv_igemm_bf16x3 (image-row 3x3)", 1, 0),
    "row.b60.n32.x3": ("igemm_f32<128,32>", 1, 0),
}

KEYS = ("id", "kind", "B", "H", "W", "C0", "C1", "N", "math", "split")
ROWS = [dict(zip(KEYS, r)) for r in _ROWS]

# labels that at least one row must carry (so that no route of the dispatch drops out of the table unnoticed)
REQUIRED_LABELS = (
    "igemm_f32<128,128>", "igemm_f32<128,64>", "igemm_f32<128,32>", "igemm_f32<128,16>", "igemm_f32<32,128>", "igemm_f32<64,128>",
    "igemm_f32<256,128> (eight waves)",
    "igemm_patch<256,128>", "igemm_patch<512,64>", "igemm_patch<256,128> + split-K reduce",
    "igemm_dma<256,128>", "igemm_dma<256,128> + split-K reduce",
    "igemm_convT_quad<32>", "igemm_convT_quad<64>",
    "igemm_convT_tap<16>", "igemm_convT_tap<32>", "igemm_convT_tap<64>",
    "conv_igemm_f32 (skinny rows)", "conv_igemm_f32 (skinny gather)", "conv_igemm_f32 (image-row 3x3)",
    "conv_igemm_bf16x3 (image-row 3x3)",
)


def fill(n, seed, dev):
    """n floats in [-0.5, 0.5) from an integer formula on the device (no RNG: the same bits on every run and every library)."""
    i = torch.arange(seed, seed + n, device=dev, dtype=torch.int64)
    return ((i * 2654435761) % 1000003).to(torch.float32) / 1000003.0 - 0.5


def conv_args(row):
    """(m2h_conv_args of the row with the pointers left null, input H, input W, output H, output W, K)."""
    from m2h import _lib, ops
    kind, B, H, W, C0, C1, N = (row[k] for k in ("kind", "B", "H", "W", "C0", "C1", "N"))
    a = _lib.ConvArgs()
    if kind == "down":
        Hi, Wi, Ho, Wo, taps = 2 * H, 2 * W, H, W, 16
        a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.os, a.slope = H, W, 2, 4, 4, 1, -1, 1, -1, 1, 0.2
    elif kind == "up":
        Hi, Wi, Ho, Wo, taps = H, W, 2 * H, 2 * W, 16
        a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.conv_transpose, a.os, a.slope = H, W, 1, 2, 2, 1, 2, 0.0
    elif kind == "c3":
        Hi, Wi, Ho, Wo, taps = H, W, H, W, 9
        a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.os, a.slope = H, W, 1, 3, 3, 1, -1, 1, -1, 1, 1.0
    else:   # lin / full: one output pixel per sample, the window is the whole image
        Hi, Wi, Ho, Wo, taps = H, W, 1, 1, H * W
        a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.os, a.slope = 1, 1, 1, H, W, 1, 0, 1, 0, 1, 1.0
    a.C0, a.C1, a.B, a.Hi, a.Wi, a.N = C0, C1, B, Hi, Wi, N
    a.Ho, a.Wo, a.ldc, a.out_mode = Ho, Wo, N, ops.OUT_NHWC
    a.operand_format = ops.FMT_MATH_BF16X3 if row["math"] == "bf16x3" else ops.FMT_MATH_FP32
    if row["split"]:
        a.operand_format |= ops.FMT_SRC_SPLIT | ops.FMT_W_SPLIT
    return a, Hi, Wi, Ho, Wo, taps * (C0 + C1)


def workspace_bytes(row):
    """What m2h_conv_igemm_workspace_bytes asks for the row (host code: needs no GPU)."""
    from m2h import _lib
    return int(_lib.load().m2h_conv_igemm_workspace_bytes(ctypes.byref(conv_args(row)[0])))


def run(row, dev):
    """Runs the row's layer once through m2h_conv_igemm_f32 with default knobs and the workspace the library asks for.
    Returns (output tensor, label, launches, workspace bytes)."""
    from m2h import _lib, ops
    kind, B, C0, C1, N = (row[k] for k in ("kind", "B", "C0", "C1", "N"))
    a, Hi, Wi, Ho, Wo, K = conv_args(row)
    x = fill(B * Hi * Wi * C0, 1, dev).view(B, Hi, Wi, C0)
    x2 = fill(B * Hi * Wi * C1, 2, dev).view(B, Hi, Wi, C1) if C1 else None
    wp = (fill(N * K, 3, dev) * (2.0 / K ** 0.5)).view(N, K)
    if row["split"]:
        x, x2, wp = ops.split32(x), (ops.split32(x2) if C1 else None), ops.split32(wp)
    keep = [x, x2, wp]
    if kind in ("down", "up"):   # the folded BatchNorm of a U-Net stage
        keep += [fill(N, 4, dev) + 1.0, fill(N, 5, dev) * 0.2]
        a.scale, a.shift = keep[3].data_ptr(), keep[4].data_ptr()
    out = torch.zeros((B, Ho, Wo, N), device=dev, dtype=torch.float32)
    a.src0, a.src1, a.wp, a.dst = x.data_ptr(), (x2.data_ptr() if C1 else None), wp.data_ptr(), out.data_ptr()
    lib = _lib.load()
    with torch.cuda.device(dev):
        wsb = int(lib.m2h_conv_igemm_workspace_bytes(ctypes.byref(a)))
        ws, _ = ops._workspace(wsb, dev)
        a.workspace, a.workspace_bytes = (ws.data_ptr() if ws is not None else None), wsb
        n0 = lib.m2h_launch_count()
        _lib.check(lib.m2h_conv_igemm_f32(ctypes.byref(a), ops._stream(out)), "m2h_conv_igemm_f32")
        launches = int(lib.m2h_launch_count() - n0)
        label = ops.last_kernel()
    return out, label, launches, wsb
