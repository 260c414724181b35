"""GPU: room_sim_kernel (csrc/room_sim.hip) on every row of tests/room_kernels.py's table through m2h_room_sim itself; every element of the
output against the float64 definition (room_ref.simulate_f64): |g - r| <= tau s, an element with s = 0 exactly 0 (kinds, taus, rows beyond
the issue, mutants: tests/room_kernels.py, pinned on the CPU by tests/test_room_kernels_cpu.py).  The 16 parameters of an RIR lie inside a
NaN-filled buffer, the output is NaN before the call and its pads are NaN afterwards; the compared count is asserted to be taps x 2; the
call is one launch, labelled room_sim.  slab, order1, order3 and dense.order5 are also run at the last place of a batch of 3 whose other rows
differ: the same bits.

Worst |g - r| / s per kind -- the float32 restatement's in the kernel's list order (CPU), the MI355X's (test_zz_report prints them with -s),
and the tau the kernel is held to, 8 x the ceiling the CPU test holds the restatement under:
  kind    restatement   MI355X      tau
  room    4.69e-7       5.01e-7     1.36e-5     (beta_ones / order4)
  dense   5.51e-7       6.32e-7     4.8e-6      (dense / dense)
Every row reports taps x 2 compared elements (slab 512 000).  dense at 600 taps (88 709 images) takes 0.47 s with its float64 reference, the
launch itself a few milliseconds, so its taps are not cut (DENSE_TAPS = 600).  No row found a kernel defect.  The 19 tests of this file take
2.7 s on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

import room_kernels as K
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
WORST = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _run(rirs):
    """m2h_room_sim on RIRs of one taps and max_order: parameters inside NaN, output NaN before the call, one launch -> [Q, taps, 2] float32"""
    params = K.pack(rirs)
    taps, order = rirs[0][5], rirs[0][6]
    assert all(r[5:] == rirs[0][5:] for r in rirs)
    Q, pad = params.shape[0], K.PAD
    pbuf = torch.full((pad + params.size + pad,), float("nan"), device=_dev(), dtype=torch.float64)
    pbuf[pad:pad + params.size] = torch.from_numpy(params.reshape(-1)).to(_dev())
    obuf = torch.full((pad + Q * taps * 2 + pad,), float("nan"), device=_dev(), dtype=torch.float32)
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    _lib.check(lib.m2h_room_sim(ctypes.c_void_p(pbuf.data_ptr() + 8 * pad), ctypes.c_void_p(obuf.data_ptr() + 4 * pad), Q, taps, -1 if order is None else order,
                                ops._stream(pbuf)), "m2h_room_sim")
    assert ops.last_kernel() == "room_sim" and lib.m2h_launch_count() == n0 + 1
    torch.cuda.synchronize()
    got = obuf.cpu().numpy()
    assert np.isnan(got[:pad]).all() and np.isnan(got[-pad:]).all()         # the pads are still NaN
    return got[pad:-pad].reshape(Q, taps, 2)


@pytest.mark.parametrize("row_id", [r["id"] for r in K.ROWS])
def test_room_sim_matches_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    taps = row["rir"][5]
    got = _run([row["rir"]])[0]
    h, s = K.reference(row)
    worst, ok, count = K.compare(got, h, s, K.tau_of(row["kind"]))
    WORST[row["kind"]] = max(WORST.get(row["kind"], (0.0, "")), (worst, row_id))
    print("%-24s %-6s worst |g-r|/s %.3e of tau %.3e  elements %d  non-zero scales %d" % (row_id, row["kind"], worst, K.tau_of(row["kind"]), count, int((s > 0).sum())))
    assert count == taps * 2 == got.size                                      # no element is left out
    assert ok, (row_id, worst, K.tau_of(row["kind"]))
    if row_id in K.BATCH_ROWS:
        batch = _run(K.batch_fillers(row) + [row["rir"]])
        assert not np.isnan(batch).any() and np.array_equal(batch[2], got)     # the same bits at the last place of a batch of 3
        assert not np.array_equal(batch[0], got) and not np.array_equal(batch[1], got)


def test_zz_report():
    for kind, (w, rid) in sorted(WORST.items()):
        print("worst |g - r| / s  %-6s %.3e (%s)   restatement's ceiling %.3e   tau %.3e" % (kind, w, rid, K.RESTATEMENT_WORST[kind], K.tau_of(kind)))
