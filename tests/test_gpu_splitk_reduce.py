"""GPU: the split-K reduce launch (csrc/conv_igemm.hip, finish_splitk) -- the row-owning kernel with all S slab loads of an item in
flight and eight channels per thread (tuning knob 42 = 0) against the one-item-per-thread kernel it replaces (knob 42 = -1), BIT FOR
BIT: the sum is 0 + s0 + s1 + ... in slab order either way, and class plane, scale / shift, activation and the hi / lo split are the
same expressions.  Through m2h_conv_igemm_f32 with knob 0 forcing the split factor of the register engine (S = 2, 3, 8: the kernel's
own instantiations; 5: its run-time loop), in both arithmetic modes, for convs and the four phases of a transposed conv, N = 20 (four
channels per thread, five items per row), 32 and 128, every destination layout (NHWC fp32, split32, de-sliced), a class-table layer,
and row counts that do not fill the last block (B = 3 on 8 x 8 grids; a 6 x 6 grid: the row decode's divisions).  Knob 43 (the
LDS-DMA engine's write-through slab stores) is checked the same way on that engine's own split-K launch."""
import ctypes

import pytest
import torch

from test_gpu_patch import _dev

pytestmark = pytest.mark.gpu

REDUCE_KNOB = 42
SLAB_WT_KNOB = 43


def _conv(x, x2, wp, Co, transposed, scale, shift, slope, fmt, S, deslice=False, cls=None, knobs=None, ws_floats=None):
    """One layer through m2h_conv_igemm_f32 with a workspace for S slabs per phase; returns (raw destination words on the CPU, label)."""
    from m2h import _lib, conv_launch, ops
    B, H, W, C0 = x.shape
    Ho, Wo = (2 * H, 2 * W) if transposed else (H // 2, W // 2)
    Hq, Wq = (H, W) if transposed else (Ho, Wo)
    out = torch.zeros((B, 16 * Ho, Wo, Co // 16) if deslice else (B, Ho, Wo, Co), device=x.device, dtype=torch.float32)
    operands = dict(wp=wp, dst=out, scale=scale, shift=shift, slope=slope, operand_format=fmt)
    a = conv_launch.conv_transpose(x, x2, Co, **operands) if transposed else conv_launch.conv(x, x2, Co, 4, 4, 2, 1, **operands)
    a.cls_table, a.cls_val = (cls[0].data_ptr(), cls[1].data_ptr()) if cls is not None else (None, None)
    a.out_mode = ops.OUT_DESLICE if deslice else ops.OUT_NHWC
    lib = _lib.load()
    n = ws_floats if ws_floats is not None else (4 if transposed else 1) * S * B * Hq * Wq * Co
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    knobs = dict(knobs or {})
    try:
        for k, v in knobs.items():
            ops.debug_set(k, v)
        with torch.cuda.device(x.device):
            _lib.check(lib.m2h_conv_igemm_f32(ctypes.byref(a), ops._stream(x)), "m2h_conv_igemm_f32")
        label = ops.last_kernel()
        torch.cuda.synchronize()
    finally:
        for k in knobs:
            ops.debug_set(k, 0)
    return out.cpu().view(torch.int32), label


def _operands(B, H, W, Ci, Co, transposed, split, seed):
    from m2h import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Ci, generator=g).to(dev)
    if transposed:
        wp = ops.pack_convT_weight((torch.randn(Ci, Co, 4, 4, generator=g) * (1.0 / (4 * Ci) ** 0.5)).to(dev))
    else:
        wp = ops.pack_conv_weight((torch.randn(Co, Ci, 4, 4, generator=g) * (1.0 / (16 * Ci) ** 0.5)).to(dev))
    scale = (torch.rand(Co, generator=g) + 0.5).to(dev)
    shift = (torch.randn(Co, generator=g) * 0.1).to(dev)
    cls = (torch.randn(9, Co, generator=g).to(dev), torch.randn(B, generator=g).to(dev))
    if split:
        x, wp = ops.split32(x), ops.split32(wp)
    return x, wp, scale, shift, cls


# (name, B, H, W of the input, Ci, Co, transposed, arithmetic / operand layout, de-sliced, class table)
#   "fp32": fp32 MFMAs; "x3": bf16x3 on fp32 operands, fp32 rows out; "split": bf16x3 on split32 operands, split32 rows out
CASES = [
    ("conv N=20", 3, 16, 16, 32, 20, False, "fp32", False, False),
    ("conv N=20 bf16x3", 3, 16, 16, 32, 20, False, "x3", False, False),
    ("conv N=32", 3, 16, 16, 32, 32, False, "fp32", False, False),
    ("conv N=128 bf16x3", 3, 16, 16, 32, 128, False, "x3", False, False),
    ("conv N=128 split32", 3, 16, 16, 32, 128, False, "split", False, False),
    ("conv N=32 de-sliced", 3, 16, 16, 32, 32, False, "fp32", True, False),
    ("conv N=32 de-sliced bf16x3", 3, 16, 16, 32, 32, False, "x3", True, False),
    ("conv N=32 class table", 3, 16, 16, 32, 32, False, "fp32", False, True),
    ("conv N=128 class table bf16x3", 3, 16, 16, 32, 128, False, "x3", False, True),
    ("conv N=128 6x6 grid", 3, 12, 12, 32, 128, False, "fp32", False, False),
    ("conv N=20 6x6 grid", 3, 12, 12, 32, 20, False, "x3", False, False),
    ("convT N=20", 3, 8, 8, 128, 20, True, "fp32", False, False),
    ("convT N=32 bf16x3", 3, 8, 8, 128, 32, True, "x3", False, False),
    ("convT N=128 split32", 3, 8, 8, 128, 128, True, "split", False, False),
    ("convT N=32 de-sliced", 3, 8, 8, 128, 32, True, "fp32", True, False),
]


@pytest.mark.parametrize("S", [2, 3, 5, 8])
@pytest.mark.parametrize("name,B,H,W,Ci,Co,transposed,mode,deslice,with_cls", CASES, ids=[c[0] for c in CASES])
def test_row_owning_reduce_keeps_every_bit(name, B, H, W, Ci, Co, transposed, mode, deslice, with_cls, S):
    from m2h import ops
    x, wp, scale, shift, cls = _operands(B, H, W, Ci, Co, transposed, mode == "split", 100 * S + Co + H)
    fmt = {"fp32": ops.FMT_MATH_FP32, "x3": ops.FMT_MATH_BF16X3,
           "split": ops.FMT_MATH_BF16X3 | ops.FMT_SRC_SPLIT | ops.FMT_W_SPLIT | ops.FMT_DST_SPLIT}[mode]
    slope = 0.0 if transposed else 0.2
    assert (16 * Ci if not transposed else 4 * Ci) // 32 >= 2 * S   # the register engine grants the forced factor (at least two k-tiles per part)
    # knob 0: the register engine at this split factor; knobs 23 / 24: not the small batches' weight-streaming kernels
    base = {0: S, 23: -1, 24: -1}
    args = (x, None, wp, Co, transposed, scale, shift, slope, fmt, S, deslice, cls if with_cls else None)
    got, label = _conv(*args, knobs={**base, REDUCE_KNOB: 0})
    again, _ = _conv(*args, knobs={**base, REDUCE_KNOB: 0})
    old, old_label = _conv(*args, knobs={**base, REDUCE_KNOB: -1})
    assert label == old_label and label.endswith("+ split-K reduce"), (label, old_label)
    assert bool((old != 0).any())
    assert torch.equal(got, old)
    assert torch.equal(again, got)


@pytest.mark.parametrize("B,H,W,Ci,Co,transposed", [
    (72, 4, 16, 256, 512, False),    # 2 x 8 outputs, M = 1152 (a ragged fifth m-tile), 20 tiles, K = 4096: the engine's launch of eight K-parts
    (32, 2, 8, 256, 256, True),      # the four phases, two n-tiles
])
def test_dma_engine_write_through_slabs_keep_every_bit(B, H, W, Ci, Co, transposed):
    """The LDS-DMA engine's own split-K launch (no knob 0; knob 36 = -1 keeps the shared-patch engine away): slab stores write-through
    (knob 43 = 0) against plain (knob 43 = -1), and the new reduce against the old one behind both."""
    from m2h import ops
    x, wp, scale, shift, _cls = _operands(B, H, W, Ci, Co, transposed, True, 7 + Co)
    fmt = ops.FMT_MATH_BF16X3 | ops.FMT_SRC_SPLIT | ops.FMT_W_SPLIT | ops.FMT_DST_SPLIT
    Hq, Wq = (H, W) if transposed else (H // 2, W // 2)
    M, phases = B * Hq * Wq, 4 if transposed else 1
    ws_floats = phases * 8 * M * Co   # room for the engine's deepest split
    args = (x, None, wp, Co, transposed, scale, shift, 0.0 if transposed else 0.2, fmt, 0)
    got, label = _conv(*args, knobs={36: -1, SLAB_WT_KNOB: 0, REDUCE_KNOB: 0}, ws_floats=ws_floats)
    assert label == "igemm_dma<256,128> + split-K reduce", label
    for wt, red in ((-1, 0), (0, -1), (-1, -1)):
        other, other_label = _conv(*args, knobs={36: -1, SLAB_WT_KNOB: wt, REDUCE_KNOB: red}, ws_floats=ws_floats)
        assert other_label == label
        assert torch.equal(got, other), (wt, red)
    assert bool((got != 0).any())
