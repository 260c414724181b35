"""Route table of the forward dispatch (conv_igemm_f32 in csrc/conv_dispatch.hip, the engines' shape rules in their own units): one row
per shape that sits on one side of a threshold the dispatch reads, with what the library did with it under default knobs -- the label of
m2h_last_kernel, the number of launches the call made, the split-K workspace m2h_conv_igemm_workspace_bytes asked for and the SHA-256 of
the output's bytes (the inputs are an integer formula, every kernel sums in a fixed order).  The facts are OBSERVED, not derived: they were
recorded once on an MI355X from the library as it stood before the retired tuning knobs (include/m2h_tuning.h) were removed, and a
refactor of the dispatch must leave every one of them as it is.  Never regenerate them from the code under test; a pull request
that means to change a route changes its row by hand and says why.  The recording run, with the kernel trace at both commits, is
profiles/forward_routes_parent_vs_branch.txt; profiles/forward_split_isa.txt has the run that checked the hashes again before they
were added here.

Row geometry (kind):
  down  Conv2d(4, 2, 1) as the U-Net runner issues it (down_args in csrc/api.hip); H x W is the OUTPUT pixel grid
  up    ConvTranspose2d(4, 2, 1) as four sub-pixel phases (up_args); H x W is the INPUT pixel grid, C1 > 0 adds a skip source
  c3    Conv2d(3, 1, 1); H x W is the image
  lin   nn.Linear over B rows of C0 floats (H = W = 1)
  full  a conv whose window is the whole H x W image: one output pixel per sample
M = B * H * W GEMM rows (per phase for `up`); `split` = sources and weights in the split32 layout (bf16x3 only).

run() is the launch the facts were recorded from; run_on() is the same launch on the caller's data in the torch layouts, for
tests/test_gpu_forward_fp64.py, which checks every row's values against float64."""
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

# id -> (label of m2h_last_kernel, launches of the call, workspace bytes, SHA-256 of the output bytes): as observed, see the module docstring
FACTS = {
    "m16.lin": ("conv_igemm_f32 (skinny rows)", 1, 0, "3ae5f1a1d39151e77b8e56961dca24b1453787ccb551b530d09633f5898672ec"),
    "m17.lin": ("conv_igemm_f32 (skinny gather)", 1, 0, "cce281c1fccae991871c36a1cd70fae6f9a9d5764c04a6f2d0fd17fa51c84fe9"),
    "m14.lin1536": ("conv_igemm_f32 (skinny rows)", 1, 0, "cee128ade3adf6702deeb141c8b55312c5d502b7bf18f9aa7d2d3ba426c6281e"),
    "m14.full": ("conv_igemm_f32 (skinny rows)", 1, 14336, "2c2cb32e095b1edbd654321ff04930c65092950e8e49f4a603962e19762e0cf2"),
    "m280.lin512": ("conv_igemm_f32 (skinny gather)", 1, 2293760, "5b282c46cec9c58ab76db74daaff34593fa87e184d4599fd2a80333aa31338b5"),
    "m280.lin1536": ("conv_igemm_f32 (skinny gather)", 1, 6881280, "8c453a86673221fdb4bf1b342a2d1b9b63725281d2b68d7b46ee0b4d56f28fa9"),
    "m32.x3": ("igemm_f32<32,128>", 1, 0, "bacb9bb3d4eeb7f8782df772327c5bc54a4dd11a33d64ed3af6ef7d8eccb075c"),
    "m33.x3": ("igemm_f32<64,128>", 1, 0, "9f81fb1ae1aa8326aa4882346d803122410336cb2e51b20e7e0a77922c4eaa59"),
    "m64.x3": ("igemm_f32<64,128>", 1, 0, "ac9f9a76d701e4b9521249cfeaffffdbe0500d06d6d4a50b6d0bd589a562885d"),
    "m65.x3": ("igemm_f32<128,128> + split-K reduce", 2, 133120, "9c060c206d7c468932ce6449247e4e19f8bf3a9a85cfc990a7b4de984b7fc144"),
    "m1024.lin": ("conv_igemm_f32 (skinny gather)", 1, 2097152, "19b0ad90f64d1a9cb9396f7db2aaffb2d7817f966330892e666e617a33fc3110"),
    "m1025.lin": ("igemm_f32<128,128> + split-K reduce", 2, 2099200, "32e5399d12b2679b0aefbfacb54ffa9b734becee28eb7f46a0bfcbf286ddaeb6"),
    "m4096.tiny": ("conv_igemm_f32 (skinny gather)", 1, 4194304, "98d5a85c4eed2015e3eaf35f430592a5ce0b03bab79bbdb41680186916567fa6"),
    "m4097.tiny": ("igemm_f32<128,64> + split-K reduce", 2, 4195328, "18a2852b9c67cdd5fea721d5e308ed73cc21a8662ae3f50cc5036f4b400c0278"),
    "m4096.w64k": ("igemm_f32<128,128> + split-K reduce", 2, 8388608, "d882b6ad1a0c5f7ead6c59f960e3add994c6567dd0771060111a7205e607a943"),
    "m4097.w64k": ("igemm_f32<128,128> + split-K reduce", 2, 8390656, "0cd2d8113d26724ac1668887a86f88c557e1cca2a3359d3fd3b0c6b7fec6af47"),
    "n16.t64": ("igemm_f32<128,16> + split-K reduce", 2, 2097152, "caae61b1d0fc3f953d560dca2b7c90531a7174c9cc4109bd8b2fe84e105be735"),
    "n20.t64": ("igemm_f32<128,32> + split-K reduce", 2, 2621440, "2c3ba2d843a39f0598d22fc47f53966256d254eed1d4d30f58c842931b541aae"),
    "n32.t64": ("igemm_f32<128,32> + split-K reduce", 2, 4194304, "c56bae346969f916f31e95d03b88cfe9f8c848da02a45e60aef56511347cb124"),
    "n36.t64": ("igemm_f32<128,64> + split-K reduce", 2, 4718592, "fb642c886023757b49a2d2d3f287f4a2210a4c4e3806c6d3c447707b806cb34e"),
    "n64.t64": ("igemm_f32<128,64> + split-K reduce", 2, 8388608, "3fe111d3c56c58ec4246e5465aa288cd9e824b752c502a561415101b684c68de"),
    "n72.t64": ("igemm_f32<128,128> + split-K reduce", 2, 9437184, "652f05c245d7177276de5752e97caeb677f77eb7fcd00cacc3546862dadb81fc"),
    "n128.t64": ("igemm_f32<128,128> + split-K reduce", 2, 16777216, "c5f94c4f99f10d9b3d5c77450b851ef0e3b02e9e6b64a778374b96786fc35cfd"),
    "n16.t256": ("igemm_f32<128,16>", 1, 0, "ade8d47ef2590cd5aebb02ebee26e324001a15c2fffddf71d468087823b05b7e"),
    "n20.t256": ("igemm_f32<128,32>", 1, 0, "251eb887f368bcc1044a309dc7f8bac50e61b175c6ddfa31e3e94ef3575d9316"),
    "n32.t256": ("igemm_f32<128,32>", 1, 0, "17f18cefab4d7439853e4442a8befc5c1bd79d0e6d4ace7a268e3eb15b41ca06"),
    "n36.t256": ("igemm_f32<128,64>", 1, 0, "212e61613bcc1d58a31ea5ec0d63f05f23b12be0fa324a91484110d740848215"),
    "n64.t256": ("igemm_f32<128,64>", 1, 0, "d75fac1be2927dc79f39e7e9e60b0e1b2285d03b913496a3923fa16d936c2e1d"),
    "n72.t256": ("igemm_f32<128,128>", 1, 0, "b9a0d8e671c63fddff533b5589a9c40855583f01e37f222123239b907279c541"),
    "n128.t256": ("igemm_f32<128,128>", 1, 0, "9ce0b2f219754a8f313584ed8754419286d07fe419bb3b6f5ac7e9ab508ab2d7"),
    "t255.lin": ("igemm_f32<128,128> + split-K reduce", 2, 33423360, "c4b238462dc43c006f855c86c1a3a51ac0280193070f2c838cd054aeade876e3"),
    "t256.lin": ("igemm_f32<128,128>", 1, 0, "09531b88324fbd14cd3199357ffc0b5adcb2746a2a16441764dffa623e76ee1b"),
    "x3.t208.plain": ("igemm_f32<128,128>", 1, 0, "16f69c58c386ddfab39972128ae11039a514f677f7b29d431f5fcdcbe32dec50"),
    "x3.t224.plain": ("igemm_f32<256,128> (eight waves)", 1, 0, "74c17fce36f955dc5910091b48312459287d497207398bd03942b98feea44356"),
    "x3.t208.split": ("igemm_dma<256,128> + split-K reduce", 2, 54525952, "0c9505671045e3dd74e4d4f5526d2a7916aa2078fc380342675fdd2b0eadf3d4"),
    "x3.t224.split": ("igemm_patch<256,128>", 1, 0, "882398d57af8d6bdeac43f8aee20b774d9c7b4cec31b9abd18635def25133cdb"),
    "x3.t208.c3": ("igemm_f32<128,128>", 1, 0, "6fda195351ba401f52a53ab8d1155d178cbbd961ea9ae92923e862b14e8ecbe9"),
    "x3.t224.c3": ("igemm_dma<256,128>", 1, 0, "56699d4fdfff6b2abf09d6c65e0daf611ea220a651108e39620bc7899b457171"),
    "x3.khalves": ("igemm_patch<256,128> + split-K reduce", 2, 33554432, "9e661ec3507106d94673254a222765b9343e3a308bfe450bedcbd8744eef46a5"),
    "up.patch64.t220": ("igemm_f32<128,64>", 1, 0, "35775e60854098a1a917e5e0a2cc02fd1fadddb037d5629676bcd5051d245ee5"),
    "up.patch64.t224": ("igemm_patch<512,64>", 1, 0, "93cf52004fbbe6fb5d7cc87a769d3987fc853037ef613d05c433bc74606e1f72"),
    "x3.n64.img4096": ("igemm_f32<128,64>", 1, 0, "3ff76e736be055bb06dd1b47de5e341afe12e708d862dde7255a77e881cc0ef3"),
    "up.n16.m32k": ("igemm_convT_tap<16>", 1, 0, "d1e8ca48b5cd635a52321c32a8b557f977255bbf953e2420b6ebad8b9c1322e7"),
    "up.n16.m57k": ("igemm_convT_tap<16>", 1, 0, "0e7c1ce27b2e4393edc37c2075c45103775813d488681c44d565f0849385fea1"),
    "up.n64.m32k": ("igemm_convT_tap<64>", 1, 0, "8dcae0d73bddc5012909f2f8432a6237cb3850e69b196e6c6d368cda42c6bc15"),
    "up.n64.m57k": ("igemm_convT_tap<64>", 1, 0, "ef055d665f069830b642340f587341f589d2f004033c8cac1e1a47d376eb01e3"),
    "up.n32.m32k.split": ("igemm_convT_tap<32>", 1, 0, "2d2b1ac3abc4fc1ee29a824dc824c3e216e711d788a7516b1827cd5871d33ae0"),
    "up.n32.m57k.split": ("igemm_convT_quad<32>", 1, 0, "d259343b5f83d522707414e3035a54e020064db166459e213214a24056971218"),
    "up.n64.m32k.split": ("igemm_convT_quad<64>", 1, 0, "038daf45d70612f4f8c472e6070e60746451093c83c8dce18f84a7d0e9b98b44"),
    "up.n64.m57k.split": ("igemm_convT_quad<64>", 1, 0, "510c86cb3ac74aaa18345db58bc374f1f4ed2b5998dd5a3458334083d20ce701"),
    "up.n64.m57k.h28": ("igemm_convT_quad<64>", 1, 0, "3e3f6339ee718546c718377277d7184f87090b8b815d2dcff7f4f0a90f9fce9c"),
    "up.n64.m57k.skip": ("igemm_convT_quad<64>", 1, 0, "ddeaeea3bf2a8d0278331057fe1115b2cd13143754e0b7de0e1cd0fe08a396b4"),
    "row.b64.n16.fp32": ("conv_igemm_f32 (image-row 3x3)", 1, 0, "f7b963aa12dcd6d72ea601c8448e5b56f7fbd5420c6b79595761cfea4add4238"),
    "row.b60.n16.fp32": ("igemm_f32<128,16>", 1, 0, "3f9a1c126fca1b64be7b0d28fb9bc9142a9cf9ed239fd455e2f7aec5790aea1e"),
    "row.b64.n32.fp32": ("conv_igemm_f32 (image-row 3x3)", 1, 0, "6012989d549b7b7025792e5500040951822269def54909f7349f089ab43c4b34"),
    "row.b60.n32.fp32": ("igemm_f32<128,32>", 1, 0, "385a1dcf383ac20ccfdc4b49f35c0c4433017a3130a7e853854226edeb08b02c"),
    "row.b64.n16.x3": ("conv_igemm_bf16x3 (image-row 3x3)", 1, 0, "8d3da345547bf6ef89527fc30f9a5d4f1f2082b282499f246f8ebce4da576fee"),
    "row.b60.n16.x3": ("igemm_f32<128,16>", 1, 0, "c288170748e2742a80ed164e4ca0be308d1466b6b0bb38b6a31e90b3e57da366"),
    "row.b64.n32.x3": ("conv_igemm_bf16x3 (image-row 3x3)", 1, 0, "f1f489694d49f5bb060a36ff627bd809c78da483b2392d6ebc9a4d49937c11c5"),
    "row.b60.n32.x3": ("igemm_f32<128,32>", 1, 0, "6ce7197771b620d21d806f130b42644a8cfa52945e8a7de5bc21d6271cebb04b"),
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


def args_of(row):
    """conv_args(row), and one more kind for the forms only tests/test_gpu_forward_fp64.py holds (no row of the table has it):
      c1    Conv2d(1, 1, 0) over an H x W image"""
    if row["kind"] != "c1":
        return conv_args(row)
    a, Hi, Wi, Ho, Wo, _ = conv_args(dict(row, kind="c3"))
    a.nth, a.ntw, a.offh, a.offw = 1, 1, 0, 0
    return a, Hi, Wi, Ho, Wo, row["C0"] + row["C1"]


def run_on(row, dev, x, x2, w, scale, shift, cls_val=None, head=None, deslice=False, dst_split=False, dst=None, ldc=None):
    """The row's layer on the caller's data: the same geometry (conv_args; args_of), default knobs and the workspace the library asks for, as run()
    -- but from fp32 CPU tensors in the torch layouts, packed by the library's own packers, so that the packers and the sub-pixel phase /
    tap map of include/m2h.h sit between the caller's reference and the output too (run() fills the packed buffer directly).
      x, x2   NCHW [B][C0][Hi][Wi] / [B][C1][Hi][Wi] (x2 None when C1 == 0)
      w       Conv2d [N][C0 + C1][kh][kw]; `up`: ConvTranspose2d [C0 + C1][N][4][4]; `lin` / `full`: [N][C0][H][W]
      scale, shift   [N] or None (the folded BatchNorm of a `down` / `up` row)
    `split` rows get ops.split32 of the sources and of the packed weights.  Forms the table's rows do not hold:
      cls_val    [B]: w carries one more input channel (C0 + 1), packed with ci_used = C0; that channel enters as the class plane
                 (ops.unet_class_table of it, times cls_val[b])
      head       (head_w [N][N], head_b [N]): the fused 1x1 head, de-sliced output, no workspace
      deslice    OUT_DESLICE: the output is [B][16 Ho][Wo][N / 16]
      dst_split  FMT_DST_SPLIT: the output rows are written in the split32 layout
      dst, ldc   a caller-owned destination on the device whose rows are ldc >= N floats apart (a column block of a wider matrix)
    Returns (output tensor on the device -- NHWC unless a form above says otherwise, label, launches, workspace bytes)."""
    from m2h import _lib, ops
    kind, B, C0, C1, N = (row[k] for k in ("kind", "B", "C0", "C1", "N"))
    a, Hi, Wi, Ho, Wo, K = args_of(row)
    assert tuple(x.shape) == (B, C0, Hi, Wi) and (x2 is None) == (C1 == 0) and (x2 is None or tuple(x2.shape) == (B, C1, Hi, Wi))

    def nhwc(t):
        return t.permute(0, 2, 3, 1).contiguous().to(dev)

    xd, x2d, wd = nhwc(x), (nhwc(x2) if C1 else None), w.contiguous().to(dev)
    keep = []
    if kind == "up":
        assert tuple(w.shape) == (C0 + C1, N, 4, 4) and cls_val is None
        wp = ops.pack_convT_weight(wd)
    elif cls_val is not None:
        assert tuple(w.shape) == (N, C0 + 1, a.nth, a.ntw) and C1 == 0
        wp = ops.pack_conv_weight(wd, ci_used=C0)
        keep += [ops.unet_class_table(wd, C0), cls_val.contiguous().to(dev)]
        a.cls_table, a.cls_val = keep[0].data_ptr(), keep[1].data_ptr()
    else:
        assert tuple(w.shape) == (N, C0 + C1, a.nth, a.ntw)
        wp = ops.pack_conv_weight(wd)
    assert wp.numel() == N * K
    if row["split"]:
        xd, x2d, wp = ops.split32(xd), (ops.split32(x2d) if C1 else None), ops.split32(wp)
    if scale is not None:
        keep += [scale.contiguous().to(dev), shift.contiguous().to(dev)]
        a.scale, a.shift = keep[-2].data_ptr(), keep[-1].data_ptr()
    if head is not None:
        keep += [head[0].contiguous().to(dev), head[1].contiguous().to(dev)]
        a.head_w, a.head_b = keep[-2].data_ptr(), keep[-1].data_ptr()
        deslice = True
    if deslice:
        a.out_mode = ops.OUT_DESLICE
    if dst_split:
        a.operand_format |= ops.FMT_DST_SPLIT
    if dst is not None:
        out, a.ldc = dst, ldc
    else:
        out = torch.zeros((B, 16 * Ho, Wo, N // 16) if deslice else (B, Ho, Wo, N), device=dev, dtype=torch.float32)
    a.src0, a.src1, a.wp, a.dst = xd.data_ptr(), (x2d.data_ptr() if C1 else None), wp.data_ptr(), out.data_ptr()
    lib = _lib.load()
    with torch.cuda.device(dev):
        wsb = 0 if head is not None else int(lib.m2h_conv_igemm_workspace_bytes(ctypes.byref(a)))
        ws, _ = ops._workspace(wsb, dev)
        a.workspace, a.workspace_bytes = (ws.data_ptr() if ws is not None else None), wsb
        n0 = lib.m2h_launch_count()
        _lib.check(lib.m2h_conv_igemm_f32(ctypes.byref(a), ops._stream(out)), "m2h_conv_igemm_f32")
        launches = int(lib.m2h_launch_count() - n0)   # (the packers and split32 above launched before n0)
        label = ops.last_kernel()
        torch.cuda.synchronize(dev)   # the operands above live until the launch is done
    return out, label, launches, wsb
