"""CPU: the table of tests/train_kernels.py reaches every cell of its coverage lists, the library's BatchNorm workspace size agrees with
the restated split count, every float32 restatement of a kernel's algorithm stays inside the family's tau against the float64 reference
on every row, and every mutant of a restatement leaves it on the rows named for it.  The last two anchor the error scales before any
GPU run: a restatement of a correct algorithm that does not fit means the scale is wrong, a mutant that fits means the row is too weak."""
import pytest
import torch

import train_kernels as K
from m2h import _lib, ops


ROW_COUNT = {"bn": 26, "gru": 87, "gru_seq": 28, "lstm": 10, "heads": 56, "loss": 18, "adam": 18}


def _ids(family):
    return [r["id"] for r in K.ROWS[family]]


@pytest.mark.parametrize("family", sorted(K.ROWS))
def test_rows_reach_every_cell(family):
    reached = {}
    for row in K.ROWS[family]:
        for c in K.CELLS[family](row):
            reached.setdefault(c, []).append(row["id"])
    missing = K.all_cells(family) - set(reached)
    assert not missing, sorted(map(str, missing))
    for c in sorted(K.all_cells(family), key=str):
        print("%-70s %s" % (c, ", ".join(reached[c][:3])))
    assert len({r["id"] for r in K.ROWS[family]}) == len(K.ROWS[family]) == ROW_COUNT[family]      # (a row taken out fails here or above)


def test_bn_rows_are_the_issue_table_and_the_library_agrees_on_the_splits():
    lib = _lib.load()
    want = {(2, 4, 0): ("one launch", 1), (255, 12, 0): ("one launch", 1), (256, 64, 0): ("one launch", 1), (257, 64, 4096): ("one launch", 4),
            (1024, 8, 4096): ("one launch", 4), (1025, 4, 4096): ("one launch", 16), (4096, 16, 4096): ("one launch", 16),
            (257, 64, 0): ("three launches", 0), (2, 4, -1): ("three launches", 0), (33, 4, -1): ("three launches", 0),
            (2081, 68, 0): ("three launches", 0), (5000, 512, 0): ("three launches", 0), (4097, 4, 4096): ("three launches", 0)}
    assert {(r["M"], r["C"], r["knob"]) for r in K.BN_ROWS} == set(want)
    for (M, C, knob), (label, R) in want.items():
        rt = K.bn_route(M, C, knob)
        assert (rt["label"], rt["R"]) == (label, R), (M, C, knob, rt)
        assert lib.m2h_bn_workspace_bytes(M, C) == rt["workspace"] == rt["splits"] * C * 12
        assert rt["rps"] * (rt["splits"] - rt["empty"]) >= M > rt["rps"] * (rt["splits"] - rt["empty"] - 1)
    assert K.bn_route(33, 4, -1)["splits"] == 2
    rt = K.bn_route(2081, 68)
    assert (rt["splits"], rt["rps"], rt["colblocks"], rt["empty"]) == (66, 32, 2, 0)
    rt = K.bn_route(5000, 512)
    assert (rt["splits"], rt["rps"], rt["empty"]) == (128, 40, 3)
    assert {s for r in K.BN_ROWS for s in [r["slope"]]} == {0.0, 0.2}
    kinds = K.bn_channel_kinds(4)
    assert set(kinds) == {"plain", "large", "const"}


def test_restated_routes():
    assert K.gru_route(14, 512, 3) == dict(fused=True, forward="gru_step", backward=["gru_gates_bwd", "gru_bwd_step", "gru_bwd_rec"])
    assert K.gru_route(14, 64, 1)["backward"] == ["gru_gates_bwd", "gru_bwd_rec"]
    assert not K.gru_route(17, 64, 2)["fused"] and not K.gru_route(14, 20, 2)["fused"]
    assert K.gru_route(17, 64, 2)["backward"] == ["gru_gates_bwd", "gru_bwd_combine"]
    assert K.GRU_STEP_MAX_ROWS == ops.GRU_STEP_MAX_ROWS
    assert K.heads_route(512, 3) == dict(load="16-byte loads", ZS=4, wgrad="policy_heads_wgrad")
    assert K.heads_route(320, 5) == dict(load="scalar loads", ZS=8, wgrad="policy_heads_wgrad")
    assert K.heads_route(64, 8) == dict(load="scalar loads", ZS=12, wgrad="tiled engine")
    assert not K.enters_grid_stride_loop(1024 * 256, K.PARTS) and K.enters_grid_stride_loop(1024 * 256 + 3, K.PARTS)
    assert not K.enters_grid_stride_loop(2048 * 256, K.ADAM_CAP) and K.enters_grid_stride_loop(2048 * 256 + 5, K.ADAM_CAP)


def _bound(g, r, s, tau, name="", row=None):
    return K.check(g, r, s, tau, K.bn_lsq(name, row["C"]) if row is not None and row["family"] == "bn" else None)


def _assert_within(family, row, got, ref, what="restatement"):
    for name, (r, s) in ref.items():
        if name not in got:
            continue
        g = torch.as_tensor(got[name])
        assert bool(torch.isfinite(g).all()), (row["id"], name)
        worst, scale, ok = _bound(g, r, s, K.TAU[family], name, row)
        assert ok, (what, row["id"], name, worst, scale)


def _rejected(family, got, ref, row=None):
    """Names of the outputs on which the bound rejects `got`."""
    bad = []
    for name, (r, s) in ref.items():
        if name in got:
            g = torch.as_tensor(got[name])
            if not bool(torch.isfinite(g).all()) or not _bound(g, r, s, K.TAU[family], name, row)[2]:
                bad.append(name)
    return bad


def _mutants_of(family, row):
    return [m for m, (f, pred) in K.MUTANT_ROWS.items() if f == family and pred(row)]


def test_every_mutant_has_rows():
    for m, (f, pred) in K.MUTANT_ROWS.items():
        assert sum(1 for r in K.ROWS[f] if pred(r)) >= 2, m
    assert set(K.MUTANT_ROWS) == set(K.BN_MUTANTS + K.GRU_MUTANTS + K.LSTM_MUTANTS + K.HEADS_MUTANTS + K.LOSS_MUTANTS + K.ADAM_MUTANTS +
                                     tuple(("seq", m) for m in K.SEQ_MUTANTS))


@pytest.mark.parametrize("row_id", _ids("bn"))
def test_bn_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.bn_inputs(row)
    got, state = K.bn_fp32(row, inp)
    ref = K.bn_reference(row, inp, state)
    _assert_within("bn", row, got, ref)
    # the figures of the large-mean channels (the bound on invstd there is tau * cond = 0.2 relative: the restated algorithms sit orders below, a
    # one-pass variance above)
    large = [c for c, k in enumerate(K.bn_channel_kinds(row["C"])) if k == "large"]
    rel = ((torch.from_numpy(got["invstd"]).double() - ref["invstd"][0]).abs() / ref["invstd"][0])[large]
    one, _ = K.bn_fp32(row, inp, K.BN_MUTANTS[0])
    rel1 = ((torch.from_numpy(one["invstd"]).double() - ref["invstd"][0]).abs() / ref["invstd"][0])[large]
    print("%s  invstd relative error on the large-mean channels: restated %.1e, one-pass %.1e" % (row_id, float(rel.max()), float(rel1.max())))
    for m in _mutants_of("bn", row):
        mg, mstate = K.bn_fp32(row, inp, m)
        bad = _rejected("bn", mg, K.bn_reference(row, inp, mstate), row)
        assert bad, (row_id, m)
    if row["M"] >= 33:
        assert {"invstd", "y"} <= set(_rejected("bn", one, ref, row)), row_id


@pytest.mark.parametrize("row_id", _ids("gru"))
def test_gru_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.gru_inputs(row)
    ref = K.gru_reference(row, inp)
    _assert_within("gru", row, K.gru_fp32(row, inp), ref)
    for m in _mutants_of("gru", row):
        assert _rejected("gru", K.gru_fp32(row, inp, m), ref), (row_id, m)


@pytest.mark.parametrize("row_id", _ids("gru_seq"))
def test_gru_sequence_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.seq_inputs(row)
    ref = K.seq_reference(row, inp)
    for name, want in K.seq_autograd64(row, inp).items():        # the reference's BPTT formulas are float64 autograd's
        assert float((ref[name][0] - want).abs().max()) <= 1e-11 * (1.0 + float(want.abs().max())), (row_id, name)
    _assert_within("gru_seq", row, K.seq_fp32(row, inp), ref)
    for m in _mutants_of("gru_seq", row):
        assert _rejected("gru_seq", K.seq_fp32(row, inp, m[1]), ref), (row_id, m)


@pytest.mark.parametrize("row_id", _ids("lstm"))
def test_lstm_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.lstm_inputs(row)
    got, state = K.lstm_fp32(row, inp)
    _assert_within("lstm", row, got, K.lstm_reference(row, inp, state))
    for m in _mutants_of("lstm", row):
        mg, ms = K.lstm_fp32(row, inp, m)
        assert _rejected("lstm", mg, K.lstm_reference(row, inp, ms)), (row_id, m)


@pytest.mark.parametrize("row_id", _ids("heads"))
def test_heads_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.heads_inputs(row)
    got, state = K.heads_fp32(row, inp)
    _assert_within("heads", row, got, K.heads_reference(row, inp, state))
    for m in _mutants_of("heads", row):
        mg, ms = K.heads_fp32(row, inp, m)
        assert _rejected("heads", mg, K.heads_reference(row, inp, ms)), (row_id, m)


@pytest.mark.parametrize("row_id", _ids("loss"))
def test_loss_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.loss_inputs(row)
    got = K.loss_fp32(row, inp)
    _assert_within("loss", row, got, K.loss_reference(row, inp, got))
    for m in _mutants_of("loss", row):
        mg = K.loss_fp32(row, inp, m)
        assert _rejected("loss", mg, K.loss_reference(row, inp, mg)), (row_id, m)
    if row["kernel"] == "ppo_loss" and row["n"] >= 8:
        assert int(K.ppo_edge_elements(inp).sum()) == 4


@pytest.mark.parametrize("row_id", _ids("adam"))
def test_adam_restatement_fits_and_mutants_do_not(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.adam_inputs(row)
    p, m, v = inp["p"], torch.zeros_like(inp["p"]), torch.zeros_like(inp["p"])
    hit = {mu: False for mu in _mutants_of("adam", row)}
    for step in range(1, K.ADAM_STEPS + 1):
        g = inp["grads"][step - 1]
        coef = K.clip_fp32(row, g)
        _assert_within("adam", row, {"coef": coef}, K.clip_reference(row, g))
        ref = K.adam_reference(row, step, p, g, m, v, coef[0])
        got = K.adam_fp32(row, step, p, g, m, v, coef[0])
        _assert_within("adam", row, got, ref)
        for mu in hit:
            hit[mu] = hit[mu] or bool(_rejected("adam", K.adam_fp32(row, step, p, g, m, v, coef[0], mu), ref))
        p, m, v = (torch.from_numpy(got[k]) for k in ("p", "m", "v"))      # the next step starts from the state this one left
    assert all(hit.values()), (row_id, hit)
