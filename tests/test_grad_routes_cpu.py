"""CPU: the gradient test table of tests/test_gpu_grad_routes.py reaches every weight-gradient route cell, and the library's own workspace
sizes (host functions, no GPU) agree with the split counts tests/grad_routes.py restates for each row -- a dispatch change that moves a
row to another block shape, split count or epilogue fails here before any GPU run."""
import ctypes
import types

import pytest

import grad_routes as G
from m2h import _lib, conv_launch, ops


def _fake(B, H, W, C):
    return types.SimpleNamespace(shape=(B, H, W, C), data_ptr=lambda: 0)


def _workspace_bytes(row):
    lib = _lib.load()
    B, H, W, C0, C1, Co, k, s, p = (row[f] for f in ("B", "H", "W", "C0", "C1", "Co", "k", "s", "p"))
    x, x2 = _fake(B, H, W, C0), (_fake(B, H, W, C1) if C1 else None)
    if row["op"] == "convT":
        return lib.m2h_convT_wgrad_workspace_bytes(ctypes.byref(conv_launch.conv_transpose_phase(x, x2, Co, 0, 0)))
    return lib.m2h_conv_wgrad_workspace_bytes(ctypes.byref(conv_launch.conv(x, x2, Co, k, k, s, p)))


def test_table_reaches_every_route_cell():
    reached = {}
    for row in G.ROWS:
        for c in G.cells(row):
            reached.setdefault(c, []).append(row["id"])
    missing = G.all_cells() - set(reached)
    assert not missing, sorted(map(str, missing))
    for c in sorted(G.all_cells(), key=str):
        print("%-55s %s" % (c, ", ".join(reached[c][:4])))
    assert sorted({r["shipped"] for r in G.ROWS if r["shipped"]}) == sorted(G.SHIPPED)
    ragged = [r for r in G.ROWS if r["shipped"] and r["shipped"].startswith("policy.")]
    assert {r["B"] for r in ragged} == {280, 37}     # the update batch and a ragged one
    assert len({r["id"] for r in G.ROWS}) == len(G.ROWS)


@pytest.mark.parametrize("row_id", [r["id"] for r in G.ROWS])
def test_row_route_and_workspace_match_the_library(row_id):
    row = G.ROWS_BY_ID[row_id]
    rt = G.route(row)
    assert not G.is_row3x3(row), "the image-row 3x3 kernels are not a route of this table"
    if row["S"] is not None:
        assert rt["S"] == row["S"], (rt["S"], row["S"])
    with ops.tuning_scope(ops.tuning_snapshot()):
        for kn, v in row["knobs"].items():
            ops.debug_set(kn, v)
        got = _workspace_bytes(row)
    assert got == rt["workspace"], (got, rt)
    assert rt["workspace"] == (4 if rt["quad"] else 1) * rt["S"] * rt["N"] * rt["Kpad"] * 4 + (4 * rt["N"] * rt["K"] * 4 if rt["quad"] else 0)


def test_restated_dispatch_sees_the_knobs():
    """The knobs the table uses change what the restatement says they change (and the library agrees, through the workspace size)."""
    lin = G.ROWS_BY_ID["i64k1.S2"]
    assert G.route(lin)["bng"] == 64 and G.route(G.ROWS_BY_ID["edge.small_m_off"])["bng"] == 128
    assert G.route(G.ROWS_BY_ID["i32k2.S9"])["kt"] == 2 and G.route(G.ROWS_BY_ID["i32k3.S4"])["kt"] == 3
    row = dict(G.ROWS_BY_ID["i128.S19"], knobs={})
    with ops.tuning_scope(ops.tuning_snapshot()):
        base = _workspace_bytes(row)
        ops.debug_set(11, 19 * 2)
        assert _workspace_bytes(row) * G.route(row)["S"] == base * 19
