"""Route table of the weight-gradient dispatch (conv_wgrad_f32 in csrc/conv_bwd.hip, the kernel families in csrc/wgrad_tiled.hip,
csrc/wgrad_row3x3.hip and csrc/wgrad_reduce.hip): one row per launch shape, with what the library did with it -- the number of launches
the call made (m2h_launch_count), the workspace its own size function asked for and the SHA-256 of the gradient's bytes (the inputs are
an integer formula, forward_routes.fill; every kernel sums in a fixed order).  The facts are OBSERVED, not derived: they were recorded
once on an MI355X from the library as it stood before conv_bwd.hip was split into one unit per kernel family, and a refactor of the
dispatch or of a kernel must leave every one of them as it is.  Never regenerate them from the code under test; a pull request that
means to change a route changes its row by hand and says why.  The recording runs (twice, same hashes) and the run that checked the
table against both libraries are in profiles/wgrad_split_isa.txt.

Two groups of rows:
  g.*    every row of tests/grad_routes.py (the tiled kernel's six block shapes x split classes, the reduce / re-layout epilogues, the
         shipped layer shapes) with the row's own knobs, through the entry its `op` names: `wgrad` -> m2h_conv_wgrad_f32 (packed
         layout), `conv` / `linear` -> m2h_conv_wgrad_torch_f32 (torch layout, no gate), `convT` -> m2h_convT_wgrad_f32 (quad)
  row.*  the image-row 3x3 kernels (3x3 / 1 / 1 over 32-channel, 32-pixel-wide images), which grad_routes.py leaves out, at three heights:
         b3h32  96 image rows, S = 24: the quarter-sum reduces, splits start mid-image
         b5h8   40 image rows, S = 10: one sum per element, image edges fall on split edges
         b3h7   21 image rows, S = 5:  ragged splits that cross image edges mid-split
         each as fp32 packed (N = 32 | 16 | 8), fp32 gated into the torch layout (slope 0), bf16x3 packed (N = 32 | 16), bf16x3 gated
         into the torch layout, the fused input gradient (m2h_conv_wgrad_dgrad_fused_f32, dy2 of 16 channels) and, with knob 21 = -1,
         the tiled kernel on the same shape (same workspace: the split count is decided by geometry alone)."""
import ctypes

import torch

import grad_routes as G
from forward_routes import fill

ROW_SIZES = (("b3h32", 3, 32, 24), ("b5h8", 5, 8, 10), ("b3h7", 3, 7, 5))   # (tag, B, H, split count S)
# (tag, entry, N, math, knobs)
_ROW_ROUTES = (("n32.fp32", "packed", 32, "fp32", {}), ("n16.fp32", "packed", 16, "fp32", {}), ("n8.fp32", "packed", 8, "fp32", {}),
               ("n32.fp32.gated", "gated", 32, "fp32", {}),
               ("n32.x3", "packed", 32, "bf16x3", {}), ("n16.x3", "packed", 16, "bf16x3", {}),
               ("n32.x3.gated", "gated", 32, "bf16x3", {}),
               ("n32.x3.fused", "fused", 32, "bf16x3", {}),
               ("n32.fp32.tiled", "packed", 32, "fp32", {21: -1}))
_ENTRY_OF_OP = {"wgrad": "packed", "conv": "torch", "linear": "torch", "convT": "quad"}


def _rows():
    out = []
    for r in G.ROWS:
        out.append(dict(id="g." + r["id"], entry=_ENTRY_OF_OP[r["op"]], B=r["B"], H=r["H"], W=r["W"], C0=r["C0"], C1=r["C1"], N=r["Co"],
                        k=r["k"], s=r["s"], p=r["p"], ci=r.get("ci", r["C0"] + r["C1"]), math="fp32", knobs=dict(r["knobs"])))
    for tag, B, H, _S in ROW_SIZES:
        for rtag, entry, N, math, knobs in _ROW_ROUTES:
            out.append(dict(id="row.%s.%s" % (tag, rtag), entry=entry, B=B, H=H, W=32, C0=32, C1=0, N=N, k=3, s=1, p=1, ci=32, math=math,
                            knobs=dict(knobs)))
    return out


ROWS = _rows()

# id -> (launches of the call, workspace bytes, SHA-256 of the gradient's bytes): as observed, see the module docstring
FACTS = {
    "g.i128.S1": (2, 327680, "199b53483be303aa4983415dbd43eebb17f9bfdc9ae106861eacf2c2f3dc2ce8"),
    "g.i128.S3": (2, 1720320, "1cfeb467feb1fa1b12b667605a9c00eac526d465043068fc6b6d5c379ab08bd0"),
    "g.i128.S11": (2, 5406720, "5dd413b13d346a36797fb97a77b63322c9ef76b353286e111dc759000186c0be"),
    "g.i128.S19": (2, 1264640, "22511b0fe23412f95ebcbc212d4dc80b19afe72d006002d542e00cf668313edd"),
    "g.i64k2.S1": (2, 73728, "29e194fac09cf97ff0d8217ec7ba9e8b9492652922b61e8aee420b848eb4c905"),
    "g.i64k2.S5": (2, 819200, "a1b7823abea6b0be115744d4728718b85c5d98d01423e451fcb67044f20b67d1"),
    "g.i64k2.S13": (2, 7340032, "08f5b5d995e7afce543a1d6ea840bd41b796f91196090cd0bfa6159ab52a38ef"),
    "g.i64k2.S26": (2, 2236416, "32ad1568e3ce62655cd2cf775ea405d1f5187eb0a9a59533f928a6247096db01"),
    "g.i64k1.S1": (2, 1048576, "dcad79c1ef994746ffd0c59d90b481e6f791458bccc3527793f8a9c10812654d"),
    "g.i64k1.S2": (2, 6291456, "ebe8b7f85f40ade6f40b2d25a9d5a44454c0be1b6efae09f9fd6971bd8f84616"),
    "g.i64k1.S14": (2, 344064, "bfe8663b1860ff87c6bb9e4950a943909e9a34baf3ce7d9c03316e630bfd24b3"),
    "g.i64k1.S23": (2, 753664, "d1562b22d78b0faa748cbe9a1628ccfd7a4577cb40e6507b8123f9566b57ddd3"),
    "g.i32k1.S1": (2, 8192, "92c500f6799f9e121cb647a22be9fd3556b8d18a10e08dcd61d71b2851609d41"),
    "g.i32k1.S3": (2, 36864, "b590dd521bd5d0991a9d10258535110b91df4ee4cf40c7328628e597fd1decbf"),
    "g.i32k1.S10": (2, 102400, "6da16b11430e105ee624255fb4617258f7b16e7a3bf99b174b8a83d9bb197c40"),
    "g.i32k1.S19": (2, 311296, "187649e49336ffb3152bf41f27af951eb9022f8fd5b22f673d980fc8914c091a"),
    "g.i32k2.S1": (2, 32768, "244f102e431f8a46a54c21ba9c08cde1cc97440c6120e2eea2e9a9acadf6d0c0"),
    "g.i32k2.S3": (2, 524288, "051c7bacaa0ddb1500d3fcac51fa2a7ba5c0e2bb281ed898e859f441cf21a284"),
    "g.i32k2.S9": (2, 516096, "82fae70a8d7a1b63f3d856711a01bd69b3eade1b67c4b32aa8105cb5c32f32fa"),
    "g.i32k2.S18": (2, 589824, "80810db53d9ffbd3ad637c222aa0a4661f80b5ae8d133e21ee1be4de4dc5c15d"),
    "g.i32k3.S1": (2, 49152, "b0f418a40d99dc87d9f3f2c2a85906523853c1202ea5fedf90ce7313df79fb4c"),
    "g.i32k3.S4": (2, 262144, "f20b401b76002120d0511649fe9bf7f8f084afc40c3bba2c617003a1e9c6d5a7"),
    "g.i32k3.S15": (2, 460800, "5998b0af1f1e0203a6ce7ef11c12b991c282d95868aee46ff9b49c117411068a"),
    "g.i32k3.S18": (2, 2654208, "b46db100cd4c225e8904576cf10b8086663f679af04e511fc61ff4e392875bab"),
    "g.edge.small_m_off": (2, 6291456, "ebe8b7f85f40ade6f40b2d25a9d5a44454c0be1b6efae09f9fd6971bd8f84616"),
    "g.edge.pad_gy": (2, 229376, "62b32d8d519bed19f746fd67ec0193454c72f7f170cb791e4870a3aee9d54df9"),
    "g.binSep.enc0.B64": (2, 20971520, "4b940417de3b897561c91569d390c4b020f60679b92c576868b5a1ebaeff401b"),
    "g.binSep.enc1.B64": (2, 16777216, "a3a320e80ac6fb011afc6ca492985fb04624efd6fc90c0b8d2e35b19ca145d80"),
    "g.binSep.enc2.B64": (2, 16777216, "24a6ea18cac54316834c561d5f832991cb05bb67a75fcfaccfe7e9e6e9b10a1f"),
    "g.binSep.enc3.B64": (2, 16777216, "4aaed3168d7b4542d478c0c5465fc3db1149de7cea996f263c50e19175b41a4b"),
    "g.binSep.enc4.B64": (2, 16777216, "611299a5dfbe64e9b1ec85610a99d7f6105a3148e4ee69093ab8c4ba091d3b57"),
    "g.binSep.dec0.B64": (2, 33554432, "1624c2c99dad401d93aaea8531b2263c20b6e9f434577af1ee00880ab264417c"),
    "g.binSep.dec1.B64": (2, 50331648, "cda17751d50584ba315d93f080fe2527d53a2db02ca6c8e248e4a54f37f48f12"),
    "g.binSep.dec2.B64": (2, 37748736, "506f26c366c26532bf63b15526a961a27b5536ba93bbe68cf421051863fc232f"),
    "g.binSep.dec3.B64": (2, 34603008, "0cd68414d97e8d3cf6d8dee9c270bff91c788e29c9d4534bb1bacbc8fe8ea9cd"),
    "g.binSep.dec4.B64": (2, 33816576, "a25bb6197d342913adadb0a5e38ca9e8f1a3179e7db7ee609b4c10c51f77ed2d"),
    "g.binSep.head.B64": (2, 8388608, "dc3723c3e39c386ba2939a3f34548641895f945f9926c5efcbed4a336b1b558e"),
    "g.bin2mono.enc0.B64": (2, 16777216, "6df98d23cce9f96d01a9da43a6655dd8c4b69977dce1488e53afaf20ee39c48b"),
    "g.bin2mono.enc1.B64": (2, 16777216, "a3a320e80ac6fb011afc6ca492985fb04624efd6fc90c0b8d2e35b19ca145d80"),
    "g.bin2mono.enc2.B64": (2, 16777216, "24a6ea18cac54316834c561d5f832991cb05bb67a75fcfaccfe7e9e6e9b10a1f"),
    "g.bin2mono.enc3.B64": (2, 16777216, "4aaed3168d7b4542d478c0c5465fc3db1149de7cea996f263c50e19175b41a4b"),
    "g.bin2mono.enc4.B64": (2, 16777216, "611299a5dfbe64e9b1ec85610a99d7f6105a3148e4ee69093ab8c4ba091d3b57"),
    "g.bin2mono.dec0.B64": (2, 33554432, "1624c2c99dad401d93aaea8531b2263c20b6e9f434577af1ee00880ab264417c"),
    "g.bin2mono.dec1.B64": (2, 50331648, "cda17751d50584ba315d93f080fe2527d53a2db02ca6c8e248e4a54f37f48f12"),
    "g.bin2mono.dec2.B64": (2, 37748736, "506f26c366c26532bf63b15526a961a27b5536ba93bbe68cf421051863fc232f"),
    "g.bin2mono.dec3.B64": (2, 34603008, "0cd68414d97e8d3cf6d8dee9c270bff91c788e29c9d4534bb1bacbc8fe8ea9cd"),
    "g.bin2mono.dec4.B64": (2, 16908288, "0a8c9ff5b3af895271480aec61f455bde1c6bb3e761d89c3311c4a2faeba2ed8"),
    "g.bin2mono.head.B64": (2, 4194304, "3277a7906f2d887c751fb4eab8fb14538d3a00cb0e91ebd7010e6a0cb98a0eba"),
    "g.audio.conv0.B280": (2, 16777216, "310e1fe0ebd19556fa44f8e100fd976caf71a490f28237885ee3fd078f2cb8d4"),
    "g.audio.conv1.B280": (2, 1048576, "af4b01c2ac738edc324ed1ea76f39c80a051b80055d8564e36bd4247f07daac3"),
    "g.audio.conv2.B280": (2, 65536, "e73a306b670d61916241498d1fa60915400a561b45a2f03c08ced906effc3985"),
    "g.audio.fc.B280": (2, 524288, "d511f957e04509e3a103ae2501efc7373cbea3523e52b860b957664edc127f58"),
    "g.visual.conv0.B280": (2, 16777216, "c1dcc7a9de89ceb9c5b60920a7952cbeaccfdd036678fb93d373e7adb5239e77"),
    "g.visual.conv1.B280": (2, 33554432, "bf1a2525119727b2e9c25cfc439fb005aaf5ad9ffb02732565c9443d939fea18"),
    "g.visual.conv2.B280": (2, 20971520, "1d43498640c06e65e0d1d7178b9c0a8e8dbc0daf2a7daa29ddf8bc50048671db"),
    "g.visual.fc.B280": (2, 18874368, "12e0ed3cf0e61e551cfc5fb09274ee36cf1a568cf71d2b52afb621dd0bf1908b"),
    "g.audio.conv0.B37": (2, 3670016, "ccd26a7a9802108c733320251b2436dc5223887b76b8b4be10021733b4815998"),
    "g.audio.conv1.B37": (2, 131072, "3281f868395f28ad9b58b470c59211db53432b97b51a9a13a2319e07de000041"),
    "g.audio.conv2.B37": (2, 32768, "14c8563c79958f0294444af815e78e870da4558d2c99ed337253d217552f2c3b"),
    "g.audio.fc.B37": (2, 262144, "88c9aac16fa3d66efd04add789fcabf33800ec1b4b7cc876cf04fa3f844dbee5"),
    "g.visual.conv0.B37": (2, 9109504, "6475ebbb3124b228287b8657c5148339022f7100bed890167f6e321ff3203ed4"),
    "g.visual.conv1.B37": (2, 7340032, "11f54a54a0599767544c9083356f7aee2c290911835d8115f5a290601e426464"),
    "g.visual.conv2.B37": (2, 3358720, "db7c99d6af25ee1a032a1b41cf64dab9859f28ef22bfffa51f15ecea0e87a788"),
    "g.visual.fc.B37": (2, 9437184, "af8cdb5a528955ce38e21fcf40e49f750cfde702d2ce0114be0c6d1e60a1d7f3"),
    "row.b3h32.n32.fp32": (2, 1179648, "85f507b3a17c82748cbb3bd4d894cf837eae90b81e8a11b28caa2c4e587d2771"),
    "row.b3h32.n16.fp32": (2, 589824, "20491f189da27ef1c53cec17a05cd4944412292e260aa417a008486059a85f63"),
    "row.b3h32.n8.fp32": (2, 294912, "87424a4755877c896cac8b894c34747fd49a9d8f69a915d8e90c9553c40db58d"),
    "row.b3h32.n32.fp32.gated": (2, 1179648, "f70d81faeb9badefe5164207db6cd3dd5a69d0e7a8c1b0e329b7bd111c08b56a"),
    "row.b3h32.n32.x3": (2, 1179648, "81e460f98005521fc803050f77a5826b4449a63dce42a00f1cd864e42b49c739"),
    "row.b3h32.n16.x3": (2, 589824, "e794267a56b2d760db41d78fd4ab1125eb51d970c9b969d35398e7bffd93d805"),
    "row.b3h32.n32.x3.gated": (2, 1179648, "d66c2477aa8a44b78d94fcda63cd8bdf75e365ddf81946b0176711ca07f08977"),
    "row.b3h32.n32.x3.fused": (2, 1179648, "de303db0b6c936efa0009d8565e9dc8e3db9c30ada6e8ec8cc2d88cdd333afe7"),
    "row.b3h32.n32.fp32.tiled": (2, 1179648, "9be4ddbaa76231c515d2105d290d149084c20626bd4b56212bb382578b3b05b4"),
    "row.b5h8.n32.fp32": (2, 491520, "dde8a30bbe240763fbbae1cdc2b6d0e6f7adfc5435c3d621765438fbf3c98c82"),
    "row.b5h8.n16.fp32": (2, 245760, "957c3b7985b799ad58ee1f59e861bdb7dc82a55ad49427363d231ee14845fbe4"),
    "row.b5h8.n8.fp32": (2, 122880, "6071f35bc0f76d68c9dd5ccb8a0ed23c7cf02675a5bbddfed75e57ce120eda99"),
    "row.b5h8.n32.fp32.gated": (2, 491520, "ac8da14b1f7727e525c149ff98e3f314d0b87288b95cb8a66b8df172817d5218"),
    "row.b5h8.n32.x3": (2, 491520, "4fa7be5c49d0be8998c147973fda3802b5c9e4741029a10de3752236f1171f24"),
    "row.b5h8.n16.x3": (2, 245760, "9892f644e475125ed95d044d1f20affd043527d6a0ff42d1f03b41bbe1e5e50f"),
    "row.b5h8.n32.x3.gated": (2, 491520, "73ed77d317493db3f13adf271c35b25d66f802a88638fc38b6fec320d9224741"),
    "row.b5h8.n32.x3.fused": (2, 491520, "0388d54fd2c1b8de030d3be80bc7587d0dd18c87335009cacd4a922e7a1acea9"),
    "row.b5h8.n32.fp32.tiled": (2, 491520, "b34769a3d8030df98c753b42ec38dbb53e768bfe8d763c4693e63d756e589331"),
    "row.b3h7.n32.fp32": (2, 245760, "3d068df517c0d8cabccc86547c803bc1adda5cc175f41576fa44a796a820fb66"),
    "row.b3h7.n16.fp32": (2, 122880, "95cbeee466c5a1dbc2faf68f24f15c528d5be9d85cba4eb6deff40c64b5db7ab"),
    "row.b3h7.n8.fp32": (2, 61440, "22398d854dd08c980502d9a78063dfa3ab145693986fbda1b06dfeb16ebf55a2"),
    "row.b3h7.n32.fp32.gated": (2, 245760, "fa694f300f3cf727819b58c0fc7e51686177dcaabdda4bfbdd443d67a80c0017"),
    "row.b3h7.n32.x3": (2, 245760, "0b63e0072aaa39698c2c9a6e46e66551a31b5542a719a1936e21d44f9f91a183"),
    "row.b3h7.n16.x3": (2, 122880, "38a3680ef37e86f62e8ad62c5df51297a8df8b04ff0d5681b7702ed15446608b"),
    "row.b3h7.n32.x3.gated": (2, 245760, "283cbe00a1e9cb0bfa48e08d57515cbab3d64bf6989cd4080f83d19c28366968"),
    "row.b3h7.n32.x3.fused": (2, 245760, "cd86ff5c6c3e279799126a3013ae83c2b32e225542616bb04c788a8de1bf726a"),
    "row.b3h7.n32.fp32.tiled": (2, 245760, "c8dac4cff00f31c304316456a1dd90d3a1999027f26f872f4d260b9868fe5943"),
}


def conv_args(row):
    """(m2h_conv_args of the row's launch with the pointers left null, output H, output W, K)."""
    from m2h import _lib
    B, H, W, C0, C1, N, k, s, p = (row[f] for f in ("B", "H", "W", "C0", "C1", "N", "k", "s", "p"))
    a = _lib.ConvArgs()
    a.C0, a.C1, a.B, a.Hi, a.Wi, a.N, a.ldc = C0, C1, B, H, W, N, N
    if row["entry"] == "quad":   # one phase of ConvTranspose2d(4, 2, 1): taps 2x2, output step 2 (the launch walks all four)
        Ho, Wo, K = 2 * H, 2 * W, 4 * (C0 + C1)
        a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.os = H, W, 1, 2, 2, -1, 0, -1, 0, 2
    else:
        Ho, Wo, K = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, k * k * (C0 + C1)
        a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.os = Ho, Wo, s, k, k, 1, -p, 1, -p, 1
    a.Ho, a.Wo = Ho, Wo
    return a, Ho, Wo, K


def workspace_bytes(row):
    """What the library's size function asks for the row (host code: needs no GPU); knob 11 (the block-count target) is the one knob it reads."""
    from m2h import _lib, ops
    lib = _lib.load()
    a = conv_args(row)[0]
    for kn, v in row["knobs"].items():
        ops.debug_set(kn, v)
    try:
        fn = lib.m2h_convT_wgrad_workspace_bytes if row["entry"] == "quad" else lib.m2h_conv_wgrad_workspace_bytes
        return int(fn(ctypes.byref(a)))
    finally:
        for kn in row["knobs"]:
            ops.debug_set(kn, 0)


def run(row, dev):
    """Runs the row's weight gradient once through its C entry, with the row's knobs and arithmetic and the workspace the library asks for.
    Returns (gradient tensor, launches, workspace bytes)."""
    from m2h import _lib, ops
    lib = _lib.load()
    entry, B, H, W, C0, C1, N, ci = (row[f] for f in ("entry", "B", "H", "W", "C0", "C1", "N", "ci"))
    a, Ho, Wo, K = conv_args(row)[:4]
    x = fill(B * H * W * C0, 1, dev).view(B, H, W, C0)
    x2 = fill(B * H * W * C1, 2, dev).view(B, H, W, C1) if C1 else None
    dy = fill(B * Ho * Wo * N, 3, dev).view(B, Ho, Wo, N)
    y = fill(B * Ho * Wo * N, 4, dev).view(B, Ho, Wo, N)          # the gate: the layer's forward output, both signs
    dy2 = fill(B * Ho * Wo * 16, 5, dev).view(B, Ho, Wo, 16)      # fused: the next conv's output gradient and its packed weight
    w2p = (fill(16 * K, 6, dev) * (2.0 / K ** 0.5)).view(16, K)
    a.src0, a.src1 = x.data_ptr(), (x2.data_ptr() if C1 else None)
    if entry == "packed":
        dw = torch.zeros((N, K), device=dev, dtype=torch.float32)
    elif entry == "quad":
        dw = torch.zeros((C0 + C1, N, 4, 4), device=dev, dtype=torch.float32)
    else:
        dw = torch.zeros((N, ci, row["k"], row["k"]), device=dev, dtype=torch.float32)
    st = ops._stream(dw)
    calls = {
        "packed": lambda: lib.m2h_conv_wgrad_f32(ctypes.byref(a), ops._ptr(dy), N, ops._ptr(dw), st),
        "torch": lambda: lib.m2h_conv_wgrad_torch_f32(ctypes.byref(a), ops._ptr(dy), N, None, 1.0, ops._ptr(dw), ci, st),
        "gated": lambda: lib.m2h_conv_wgrad_torch_f32(ctypes.byref(a), ops._ptr(dy), N, ops._ptr(y), 0.0, ops._ptr(dw), ci, st),
        "fused": lambda: lib.m2h_conv_wgrad_dgrad_fused_f32(ctypes.byref(a), ops._ptr(dy2), ops._ptr(w2p), ops._ptr(y), 0.0, ops._ptr(dw), ci, st),
        "quad": lambda: lib.m2h_convT_wgrad_f32(ctypes.byref(a), ops._ptr(dy), N, ops._ptr(dw), st),
    }
    for kn, v in row["knobs"].items():
        ops.debug_set(kn, v)
    try:
        with torch.cuda.device(dev), ops.math_scope(ops.MATH_BF16X3 if row["math"] == "bf16x3" else ops.MATH_FP32):
            wsb = int((lib.m2h_convT_wgrad_workspace_bytes if entry == "quad" else lib.m2h_conv_wgrad_workspace_bytes)(ctypes.byref(a)))
            ws, _ = ops._workspace(wsb, dev)
            a.workspace, a.workspace_bytes = ws.data_ptr(), wsb
            n0 = lib.m2h_launch_count()
            _lib.check(calls[entry](), "weight gradient (%s)" % entry)
            launches = int(lib.m2h_launch_count() - n0)
            torch.cuda.synchronize(dev)
    finally:
        for kn in row["knobs"]:
            ops.debug_set(kn, 0)
    return dw, launches, wsb
